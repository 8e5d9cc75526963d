"""Parity across the f32 amplitude range, subnormal to overflow, under the test-only SIMT interpreter (tests/hostsim).

Every other parity test drives int16-range signals, yet process_frame takes any f32 (ref: src/denoise.rs:86-90) and the kernels make
decisions that depend on magnitude: the certified coarse pitch search (k_pitch) is certified for "ordinary values"
only and sends a 16-stream block elsewhere -- to the full search -- outside them.  Here the streams of edge_streams.make_scale_streams
(one scale per aligned block, 2^-140 .. 2^62, transitions, a mixed block) are checked against the oracle on every frame: the certified
search's pair, survivors' sums and pitch index bit for bit, both regimes present on both sides of both of its crossings, and the audio,
VAD and gains under the bars of edge_streams.check_scale_outputs, through several ways of running a frame and through export and import."""
import numpy as np
import pytest

from edge_streams import ADVISOR_EXP, check_scale_outputs, make_scale_streams
from test_pitch_certified import _run

T, SWITCH = 6, 3
# the grid thinned for the interpreter's pace, adjacent scales kept on both sides of both crossings of the certified search (measured:
# 6 frames here: full at 2^-32, certified from 2^-31 to 2^4, both at 2^5, full from 2^6; the GPU suite runs every scale of SCALE_EXP)
SCALES = (-140, -130, -64, -40, -34, -32, -31, -30, -28, -15, 0, 2, 4, 5, 6, 8, 17, 24, 40, 50, 60, 62)
WANT = ("out", "pitch", "branch", "vad", "gains")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _block(names, name):
    return slice(16 * names.index(name), 16 * names.index(name) + 16)


@pytest.fixture(scope="module")
def sweep(oracle_mod, weights_bytes):
    x, exp, names = make_scale_streams(T, SWITCH, SCALES)
    ref = oracle_mod.run_streams(oracle_mod.Model(weights_bytes), x, want=WANT)
    ref32 = oracle_mod.run_streams(oracle_mod.Model(weights_bytes, f32_fft=True), x, want=WANT)
    return x, exp, names, ref, ref32


@pytest.fixture(scope="module")
def one_frame_run(hostsim_lib, sweep):
    """The sweep in one-frame calls (the fused back end on a small batch), with every frame's taps."""
    import nnnoiseless_amd as nn
    x = sweep[0]
    S = x.shape[0]
    bd = nn.BatchDenoiser(S, lib=hostsim_lib)
    out, vad = np.empty_like(x), np.empty((S, T), np.float32)
    gains, pitch, branch = np.empty((S, T, 22), np.float32), np.empty((S, T), np.int32), np.empty((S, T), np.int32)
    for t in range(T):
        o, v = bd.process(x[:, t:t + 1])
        out[:, t], vad[:, t] = o[:, 0], v[0]
        gains[:, t], pitch[:, t], branch[:, t] = bd.tap("g"), bd.tap("pitch")[:, 0], bd.tap("branch")[:, 0]
    return out, vad, gains, pitch, branch


def oracle_lags(oracle_mod, weights_bytes, x):
    """[S, T]: how many of the 147 coarse correlations the oracle computes as numbers (not NaN) -- all of them but where huge values make
    inf - inf or 0 x inf -- which is how many the full search leaves in the kernel's tap."""
    om = oracle_mod.Model(weights_bytes)
    n = np.empty(x.shape[:2], np.int32)
    for s in range(x.shape[0]):
        st = oracle_mod.State(om)
        for t in range(x.shape[1]):
            st.process_frame(x[s, t])
            n[s, t] = (~np.isnan(st.taps()["xcorr1"])).sum()
    return n


def regimes(counts, lags, names, exps):
    """Per scale of the grid: "full" (the block took the full search on every frame: every stream kept every lag the oracle has a number
    for), "cert" (it never did) or "both"."""
    res = {}
    for k in exps:
        b = _block(names, f"2^{k}")
        full = (counts[b] == lags[b]).all(axis=0)
        res[k] = "full" if full.all() else "cert" if not full.any() else "both"
    return res


def check_crossings(reg):
    """The certified scales form one band of the grid and the full search holds on every frame outside it, but for at most one scale on
    either edge whose streams or frames fall on both sides (a crossing inside the grid): each crossing is bracketed by adjacent scales of
    the grid, certified on one side, full on the other.  Returns the pairs (last full, first certified), (last certified, first full)."""
    ks = sorted(reg)
    cert = [i for i, k in enumerate(ks) if reg[k] == "cert"]
    lo, hi = cert[0], cert[-1]
    assert cert == list(range(lo, hi + 1)), reg
    lo_f = lo - 1 if lo >= 1 and reg[ks[lo - 1]] == "full" else lo - 2
    hi_f = hi + 1 if hi + 1 < len(ks) and reg[ks[hi + 1]] == "full" else hi + 2
    assert lo_f >= 0 and hi_f < len(ks), reg
    assert all(reg[k] == "full" for k in ks[:lo_f + 1] + ks[hi_f:]), reg
    return (ks[lo_f], ks[lo]), (ks[hi], ks[hi_f])


@pytest.fixture(scope="module")
def counts(hostsim_lib, oracle_mod, weights_bytes, sweep):
    import nnnoiseless_amd as nn
    return _run(nn, oracle_mod, weights_bytes, sweep[0], lib=hostsim_lib), oracle_lags(oracle_mod, weights_bytes, sweep[0])


def test_certified_search_across_scales(counts, sweep):
    """The pair, every survivor's sum and the pitch index as the oracle's on every frame of every scale (in _run), and both regimes of the
    search where they belong: the int16 and unit-range blocks certify, 2^-40 and 2^17 take the full search, and the grid brackets both
    crossings with adjacent scales (a guard change that moves a crossing off the grid fails here)."""
    x, exp, names, ref, _ = sweep
    counts, lags = counts
    reg = regimes(counts, lags, names, SCALES)
    print("certified search by scale:", reg)
    assert reg[0] == "cert" and reg[-15] == "cert", reg
    assert reg[-40] == "full" and reg[17] == "full", reg
    quiet, loud = check_crossings(reg)
    print("crossings: full at 2^%d, certified from 2^%d to 2^%d, full from 2^%d" % (quiet + loud))
    # one extreme stream sends its 15 int16 neighbours to the full search
    b = _block(names, "mixed")
    assert (counts[b] == lags[b]).all()


def test_advisor_stream_sits_on_the_quiet_guard(oracle_mod, weights_bytes, sweep):
    """The "advisor" block is what it says: on the second loud frame |x4|^2 (from the oracle's x_lp, x4 = x_lp[384::2]) lies just above the
    certified search's quiet guard 2^-60 while the older part of the buffer sits near 2^-116."""
    x, _, names, _, _ = sweep
    om = oracle_mod.Model(weights_bytes)
    blk = x[_block(names, "advisor")]
    for s in range(16):
        st = oracle_mod.State(om)
        for t in range(SWITCH + 2):
            st.process_frame(blk[s, t])
        xl = st.taps()["xlp"].astype(np.float64)
        xx, past = (xl[384::2] ** 2).sum(), np.abs(xl[:192]).max()
        if s == 7:   # the silent stream of make_streams
            assert xx == 0.0
            continue
        assert 2.0 ** -60 <= xx <= 2.0 ** -58, (s, np.log2(xx), ADVISOR_EXP[s])
        assert 0.0 < past < 2.0 ** -100, (s, past)


def test_outputs_against_the_oracle(hostsim_lib, sweep, one_frame_run):
    """Pitch exact, VAD and gains within the oracle's own f32 / f64 spread, audio within 1e-4 of the stream's peak on unflipped frames,
    non-finite values where the oracle has them; the sweep in one call gives the bits of the one-frame calls."""
    import nnnoiseless_amd as nn
    from conftest import flip_stats
    x, exp, names, ref, ref32 = sweep
    out, vad, gains, pitch, branch = one_frame_run
    excused, flips = check_scale_outputs(out, vad, gains, pitch, branch, ref, ref32)
    fin = np.isfinite(ref["out"]).all(axis=(1, 2))
    print("flips (stream, frame, bands):", flips)
    print("flips:", flip_stats(branch[fin], out[fin], {k: ref[k][fin] for k in ("branch", "out")}, {k: ref32[k][fin] for k in ("branch", "out")}))
    bd = nn.BatchDenoiser(x.shape[0], lib=hostsim_lib)
    o, v = bd.process(x)
    assert np.array_equal(_bits(o), _bits(out)) and np.array_equal(_bits(v.T), _bits(vad))
    # the mixed block took the full search: its 15 int16 streams are those of the homogeneous block bit for bit
    m, h = _block(names, "mixed"), _block(names, "2^0")
    keep = [s for s in range(16) if s != 5]
    assert np.array_equal(_bits(out[m][keep]), _bits(out[h][keep])) and np.array_equal(_bits(vad[m][keep]), _bits(vad[h][keep]))


def test_export_import_at_scale(hostsim_lib, sweep, one_frame_run):
    """Streams exported after SWITCH frames and imported into a batch of another size, group length and block layout (2^-140 beside 2^60
    in one block) continue bit for bit: import rebuilds the decimated ring, x_lp[0] and the filtered sample from the record, and a
    rebuild that is not the kernels' own arithmetic would show on subnormal and huge values first."""
    import nnnoiseless_amd as nn
    x, exp, names, _, _ = sweep
    out, vad = one_frame_run[:2]
    src = np.concatenate([np.arange(S.start, S.stop) for S in (_block(names, n) for n in ("2^-140", "2^-15", "2^40", "2^60", "sub0"))])
    a = nn.BatchDenoiser(len(src), lib=hostsim_lib)   # (a stream's bits do not depend on its neighbours: the sweep's own batch need not run)
    a.process(x[src, :SWITCH])
    rec = a.export_streams(range(len(src)))
    rng = np.random.default_rng(7)
    S2 = len(src) + 7
    dst = rng.permutation(S2)[:len(src)]
    b = nn.BatchDenoiser(S2, lib=hostsim_lib, max_group_frames=2)
    b.process(np.zeros((S2, 1, 480), np.float32))
    b.import_streams(dst, rec)
    y = np.zeros((S2, T - SWITCH, 480), np.float32)
    y[dst] = x[src, SWITCH:]
    o, v = b.process(y)
    assert np.array_equal(_bits(o[dst]), _bits(out[src, SWITCH:])), np.argwhere(_bits(o[dst]) != _bits(out[src, SWITCH:]))[:8]
    assert np.array_equal(_bits(v[:, dst].T), _bits(vad[src, SWITCH:]))
