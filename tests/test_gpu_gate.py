"""The VAD gate (include/nnn_gate.h) on the MI355X: the checks of tests/test_hostsim_gate.py on the real kernels,
many blocks, torch tensors on a stream of torch's, and VadGate.process end to end behind the denoiser on the golden recording -- all bit
for bit against the NumPy restatement."""
import numpy as np
import pytest

import gate_cases as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    return gc.TorchMem()


@pytest.mark.parametrize("S, T", gc.SHAPES)
def test_against_the_restatement(gpu_lib, mem, S, T):
    gc.check_restatement(gpu_lib, mem, S, T, rots=(0, 1, 2, 3) if S < 70 else (0, 3))


def test_many_blocks(gpu_lib, mem):
    """4096 x 3: 1920 blocks of k_gate_apply, sixteen of k_gate_scan."""
    gc.check_restatement(gpu_lib, mem, 4096, 3, rots=(1,))


def test_chunking(gpu_lib, mem):
    gc.check_chunking(gpu_lib, mem)


def test_in_place_equals_out_of_place(gpu_lib, mem):
    gc.check_in_place(gpu_lib, mem)


def test_layout_and_formats(gpu_lib, mem):
    gc.check_layout(gpu_lib, mem)


def test_transparency_and_mute(gpu_lib, mem):
    gc.check_transparency(gpu_lib, mem)


def test_ramp(gpu_lib, mem):
    gc.check_ramp(gpu_lib, mem)


def test_live_mask(gpu_lib, mem):
    gc.check_live(gpu_lib, mem)


def test_reset_set_params_export_import(gpu_lib, mem):
    gc.check_state(gpu_lib, mem)


def test_host_call(gpu_lib, mem):
    gc.check_host_call(gpu_lib, mem)


def test_refusals(gpu_lib, mem):
    gc.check_refusals(gpu_lib, mem)


def test_torch_tensors_on_torchs_stream(gpu_lib):
    """Audio, VAD and the live mask are torch tensors made by kernels on a stream of torch's; VadGate.apply enqueues behind them on that
    stream, in place on a permuted view of the batch's [T][S][480] that starts at an odd float, and torch goes on working with the
    result on the same stream."""
    import torch
    S, T = 70, 5
    par = gc.params(S, 2)
    x, v = gc.audio(61, S, T), gc.vad_rows(62, T, par["threshold"])
    live = (np.arange(S) % 5 != 2).astype(np.uint8)
    g, rs = gc.gate(gpu_lib, S, 8, par), gc.Restated(S, 8, par)
    dev = torch.device("cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        flat = torch.cat([torch.zeros(1, device=dev), torch.from_numpy(x).to(dev).permute(1, 0, 2).reshape(-1)])[1:]
        a = flat.view(T, S, gc.FRAME).permute(1, 0, 2)                 # [S][T][480] over [T][S][480]
        tv = torch.from_numpy(v).to(dev) * 1.0
        tl = torch.from_numpy(live).to(dev)
        assert a.data_ptr() % 16 == 4
        out, op = g.apply(a, tv, live=tl, want_open=True)
        assert out is a
        total = out[torch.from_numpy(live != 0).to(dev)].abs().sum()   # (torch goes on with the result on its stream)
    st.synchronize()
    wy, wo = rs.apply(x, v, live=live, base=x)
    wo[:, live == 0] = 0                                               # (the mirror hands back zeros where nothing was written)
    gc.assert_same(out.cpu().numpy(), wy), gc.assert_same(op.cpu().numpy(), wo)
    gc.assert_records(g, rs)
    assert np.isclose(float(total), np.abs(wy[live != 0].astype(np.float64)).sum(), rtol=1e-5)
    # out of place into a second tensor of the same strides
    with torch.cuda.stream(st):
        x2 = torch.from_numpy(x).to(dev).permute(1, 0, 2).contiguous().permute(1, 0, 2)
        out2 = g.apply(x2, tv, out=torch.empty_like(x2))
    st.synchronize()
    gc.assert_same(out2.cpu().numpy(), rs.apply(x, v)[0])
    g.close()


def test_torch_tensors_on_the_default_stream(gpu_lib):
    """The caller sets no stream: torch's current stream is its default stream, whose handle 0 the C ABI reads as "the object's own
    stream".  VadGate.apply must still run behind the kernels that make audio, VAD and mask -- here at the end of a chain of matrix
    products that keeps the default stream busy for milliseconds -- and ahead of torch's next kernels there, twice in a row (the second
    call reads what the first left), in place and out of place."""
    import torch
    S, T = 70, 5
    par = gc.params(S, 1)
    x, v = gc.audio(71, S, T), gc.vad_rows(72, T, par["threshold"])
    live = (np.arange(S) % 4 != 1).astype(np.uint8)
    g, rs = gc.gate(gpu_lib, S, 8, par), gc.Restated(S, 8, par)
    dev = torch.device("cuda")
    assert torch.cuda.current_stream().cuda_stream == 0
    hx, hv, hl = torch.from_numpy(x).to(dev), torch.from_numpy(v).to(dev), torch.from_numpy(live).to(dev)
    torch.cuda.synchronize()
    m = torch.rand(2048, 2048, device=dev)
    for _ in range(30):
        m = torch.tanh(m @ m)
    zero = m.sum() * 0.0                                               # (0.0, known only when the chain has run)
    a = hx + zero                                                      # fresh memory, written behind the chain
    tv, tl = hv + zero, hl + zero.to(torch.uint8)
    handles, device_call = [], g.apply_device
    g.apply_device = lambda *args, **kw: (handles.append(kw["hip_stream"]), device_call(*args, **kw))[1]
    out, op = g.apply(a, tv, live=tl, want_open=True)
    got, got_open = out.clone(), op.clone()                            # torch's next kernels on the default stream
    b = torch.full_like(a, float(gc.SENT))
    out2 = g.apply(hx + zero, tv, out=b)
    got2 = out2.clone()
    torch.cuda.synchronize()
    assert out is a and out2 is b
    # (whether an unordered call shows in the bits depends on which hardware queues the two streams land on; that the library was
    # never handed handle 0 does not)
    assert len(handles) == 2 and all(h not in (0, None) for h in handles), handles
    wy, wo = rs.apply(x, v, live=live, base=x)
    wo[:, live == 0] = 0
    gc.assert_same(got.cpu().numpy(), wy, "in place on the default stream"), gc.assert_same(got_open.cpu().numpy(), wo)
    gc.assert_same(got2.cpu().numpy(), rs.apply(x, v)[0], "out of place on the default stream")
    gc.assert_records(g, rs)
    g.close()


def test_process_end_to_end(gpu_lib, golden_io):
    """VadGate.process on a 16-stream batch over 60 frames of the golden recording in three calls, streams 3 and 9 held during the second:
    the result equals the restatement applied to BatchDenoiser.process's own output and VAD (a second batch run the same way), and what
    the held streams own stays the sentinel.  The thresholds lie halfway between the smallest and the largest VAD value that run returns for
    the stream, so every gate opens, and those without grace and look-back (open_n = voiced_n) close as well."""
    import nnnoiseless_amd as nn
    from nnnoiseless_amd.gate import VadGate
    S, T, calls = 16, 20, 3
    inp, _ = golden_io
    x = np.stack([inp[2 * s:2 * s + T * calls] for s in range(S)]).astype(np.float32)      # [S, 60, 480]
    held = [3, 9]

    def run(fn):
        b = nn.BatchDenoiser(S, lib=gpu_lib)
        res = []
        for c in range(calls):
            if c == 1:
                b.hold_streams(held)
            if c == 2:
                b.resume_streams(held)
            res.append(fn(b, c, x[:, c * T:(c + 1) * T]))
        b.close()
        return res

    def plain(b, c, xc):
        out, vad = np.full_like(xc, gc.SENT), np.full((T, S), -1.0, np.float32)
        b.process(xc, out=out, vad=vad)
        return out, vad

    ref = run(plain)
    seen = np.concatenate([ref[0][1], ref[2][1]])                      # (calls in which every stream took part)
    lo, hi = seen.min(axis=0), seen.max(axis=0)
    thr = (lo + (hi - lo) * np.float32(0.5)).astype(np.float32)        # halfway between the smallest and the largest value of each stream
    assert ((seen >= thr).any(axis=0) & (seen < thr).any(axis=0)).all() and (thr >= 0).all() and (thr <= 1).all(), "the recording's VAD does not vary"
    par = {"threshold": thr, "grace": np.arange(S) % 2, "lookback": np.array([0, 1, 2, 3])[np.arange(S) % 4], "level": np.array([0.0, 0.1], np.float32)[np.arange(S) % 2]}
    g, rs = VadGate(S, 3, lib=gpu_lib), gc.Restated(S, 3, par)
    g.set_params(par["threshold"], par["grace"], par["lookback"], par["level"])

    def gated(b, c, xc):
        out, vad = np.full_like(xc, gc.SENT), np.full((T, S), -1.0, np.float32)
        o2, v2, op = g.process(b, xc, out=out, vad=vad, want_open=True)
        assert o2 is out and v2 is vad
        return out, vad, op

    got = run(gated)
    opens = []
    for c in range(calls):
        live = np.ones(S, np.uint8)
        if c == 1:
            live[held] = 0
        wy, wo = rs.apply(ref[c][0], ref[c][1], live=live, base=ref[c][0])
        wo[:, live == 0] = 0
        gc.assert_same(got[c][1], ref[c][1], f"call {c} vad")
        gc.assert_same(got[c][0], wy, f"call {c} audio"), gc.assert_same(got[c][2], wo, f"call {c} open")
        opens.append(wo[:, live == 1])
    assert (got[1][0][held] == gc.SENT).all() and (got[1][1][:, held] == -1.0).all()
    allo = np.concatenate([opens[0], opens[2]])
    plain_gate = (par["grace"] == 0) & (par["lookback"] == 0)
    assert (allo == 1).any(axis=0).all() and (allo == 0).any(axis=0)[plain_gate].all() and plain_gate.sum() == 4, "the gates open and close"
    print(f"streams whose gate both opened and closed: {int(((allo == 1).any(axis=0) & (allo == 0).any(axis=0)).sum())} of {S}")
    assert any((got[c][0] != ref[c][0]).any() for c in range(calls))
    gc.assert_records(g, rs)
    g.close()
