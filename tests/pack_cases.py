"""What the file packer's tests share (test_hostsim_pack.py under the SIMT interpreter, test_gpu_pack.py on the GPU library): the files,
the arenas, the yardstick and the checks.  The yardstick of a file is the SAME library's lone run -- a fresh batch of `channels` streams
and process_pcm(..., channels, discard_first=True) over the file's whole frames, the reference CLI's loop (src/nnnoiseless.rs:301-331) --
so every comparison is bit for bit, with no tolerance and no excused case.
"""
import numpy as np

FRAME = 480
CANARY_I16 = np.int16(-12345)
CANARY_F32 = np.float32(-12345.0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def to_i16(y):
    """round half away from zero in float64, then the clamp: what the CLI's writers do to a float sample."""
    y = np.asarray(y, np.float64)
    return np.clip(np.sign(y) * np.floor(np.abs(y) + 0.5), -32768, 32767).astype(np.int16)


def make_files(frames, channels=1, seed=0, tail=7, loud=()):
    """One float32 array [F * 480 + tail_i, channels] per entry of `frames`, values in the int16 range on integers (so that an int16
    copy is exact): a tone in noise, every file its own; files in `loud` are full-scale square waves that reach the output clamp.
    tail_i = a few samples of partial frame behind the last whole frame, different from file to file."""
    rng = np.random.default_rng(seed)
    out = []
    for i, F in enumerate(frames):
        n = F * FRAME + (tail + 3 * i) % FRAME
        t = np.arange(n)[:, None]
        f = rng.uniform(100.0, 6000.0, (1, channels))
        x = 7000.0 * np.sin(2 * np.pi * f * t / 48000.0) + 400.0 * rng.standard_normal((n, channels))
        if i in loud:
            x = 32767.0 * np.sign(np.sin(2 * np.pi * 220.0 * t / 48000.0) + 1e-9) * np.ones((1, channels))
        out.append(np.clip(np.rint(x), -32768, 32767).astype(np.float32))
    return out


def lone(lib, x, channels, fmt_i16=False, floors=None, link=None):
    """The yardstick: (audio [(F - 1) * 480, channels], vad [F, channels]) of ONE file processed alone.  x: [n, channels] float32 in
    the int16 range (fmt_i16: handed to the library as int16, output int16)."""
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import pcm
    F = x.shape[0] // FRAME
    dt = np.int16 if fmt_i16 else np.float32
    if F == 0:
        return np.zeros((0, channels), dt), np.zeros((0, channels), np.float32)
    bd = nn.BatchDenoiser(channels, lib=lib)
    if floors is not None:
        bd.set_gain_floor(list(range(channels)), floors)
    if link is not None:
        bd.set_channel_link(channels, link)
    fmt = pcm.PCM_I16 if fmt_i16 else pcm.PCM_F32
    o, v = bd.process_pcm(x[None, :F * FRAME].astype(dt), fmt, channels, discard_first=True)
    bd.close()
    return o[0].copy(), v.copy()


class Lone:
    """Lone runs computed once and shared (a key is the file's index in its set and how it was run)."""

    def __init__(self, lib, files, channels):
        self.lib, self.files, self.channels, self.memo = lib, files, channels, {}

    def __call__(self, i, fmt_i16=False):
        k = (i, fmt_i16)
        if k not in self.memo:
            self.memo[k] = lone(self.lib, self.files[i], self.channels, fmt_i16)
        return self.memo[k]


def in_bytes(x, fmt):
    """A file's samples (float32 on integers in the int16 range, [n, C]) as the bytes of input format `fmt`, and the float32 samples
    the library must make of them (the numpy restatement of src/nnnoiseless.rs:189-227)."""
    from nnnoiseless_amd import pcm
    rng = np.random.default_rng(x.size)
    i16 = x.astype(np.int16).reshape(-1)
    if fmt == pcm.PCM_F32:
        return x.reshape(-1).astype(np.float32).view(np.uint8), x
    if fmt == pcm.PCM_I16:
        return i16.view(np.uint8), x
    if fmt == pcm.PACK_I32:   # the low 16 bits are dropped by >> 16
        s = (i16.astype(np.int32) << 16) | rng.integers(0, 1 << 16, i16.size, dtype=np.int32)
        return s.view(np.uint8), (s >> 16).astype(np.float32).reshape(x.shape)
    if fmt == pcm.PACK_I24:   # three bytes a sample, little-endian; the low byte is dropped by >> 8
        s = (i16.astype(np.int32) << 8) | rng.integers(0, 1 << 8, i16.size, dtype=np.int32)
        b = np.stack([(s & 255), (s >> 8) & 255, (s >> 16) & 255], axis=1).astype(np.uint8).reshape(-1)
        return b, (s >> 8).astype(np.float32).reshape(x.shape)
    if fmt == pcm.PACK_F32_WAV:
        u = (x.reshape(-1) / np.float32(32768.0)).astype(np.float32)
        return u.view(np.uint8), (u * np.float32(32767)).astype(np.float32).reshape(x.shape)
    raise ValueError(fmt)


def build_arenas(files, channels, in_fmt, out_i16, gap=5, lead=3):
    """The files laid into one input arena at odd element offsets with gaps between them, and the output / VAD arenas pre-filled with a
    canary, their ranges likewise at odd offsets with gaps.  Returns (in_arena uint8, out_arena, vad_arena, table, want_in) -- table =
    [(in_off, n, out_off, vad_off)] in elements, want_in[i] = the float32 samples file i converts to."""
    from nnnoiseless_amd import _ffi
    es = _ffi.PACK_ELEM_BYTES[in_fmt]
    rng = np.random.default_rng(99)
    parts, table, want_in = [], [], []
    pos_in, pos_out, pos_vad = lead, lead, 1   # (elements)
    parts.append(rng.integers(0, 256, lead * es, dtype=np.uint8))
    for i, x in enumerate(files):
        b, w = in_bytes(x, in_fmt)
        F = x.shape[0] // FRAME
        table.append((pos_in, x.shape[0], pos_out, pos_vad))
        want_in.append(w)
        g = gap + 2 * (i % 2)   # odd gaps: the next file begins on an odd element whatever this one's length
        parts += [b, rng.integers(0, 256, g * es, dtype=np.uint8)]
        pos_in += x.shape[0] * channels + g
        pos_out += max(F - 1, 0) * FRAME * channels + g
        pos_vad += F * channels + 1 + i % 2
    in_arena = np.concatenate(parts)
    pad = (-in_arena.size) % 4
    in_arena = np.concatenate([in_arena, np.zeros(pad, np.uint8)])
    out_arena = np.full(pos_out + 8, CANARY_I16 if out_i16 else CANARY_F32, np.int16 if out_i16 else np.float32)
    vad_arena = np.full(pos_vad + 4, CANARY_F32, np.float32)
    return in_arena, out_arena, vad_arena, table, want_in


def in_view(in_arena, in_fmt):
    """The byte arena as an array of the format's element type where numpy has one (the library only wants the bytes)."""
    from nnnoiseless_amd import pcm
    dt = {pcm.PCM_F32: np.float32, pcm.PCM_I16: np.int16, pcm.PACK_I32: np.int32, pcm.PACK_F32_WAV: np.float32}.get(in_fmt)
    return in_arena if dt is None else in_arena.view(dt)


def run_packed(lib, files, channels, n_streams, step_frames, in_fmt=None, out_i16=False, order=None, configure=None, packer=None):
    """The files through a packer over canary-filled arenas.  order = a permutation: the list handed to the packer is files[order]
    (arena positions stay with the file).  Returns (outs, vads, summary, want_in) in the ORIGINAL file order, after checking that every
    byte of the output arenas outside the files' ranges still holds the canary.  configure(batch) runs on the fresh batch."""
    import nnnoiseless_amd as nn
    from nnnoiseless_amd import pcm
    in_fmt = pcm.PCM_F32 if in_fmt is None else in_fmt
    in_arena, out_arena, vad_arena, table, want_in = build_arenas(files, channels, in_fmt, out_i16)
    order = list(range(len(files))) if order is None else list(order)
    own = packer is None
    if own:
        bd = nn.BatchDenoiser(n_streams, lib=lib)
        if configure:
            configure(bd)
        packer = pcm.FilePacker(bd, channels, step_frames)
    s = packer.run_arena(in_view(in_arena, in_fmt), in_fmt, out_arena, vad_arena, [table[i] for i in order])
    if own:
        assert packer.batch.num_held() == 0
        packer.close()
        bd.close()
    outs, vads = [], []
    seen_out, seen_vad = np.zeros(out_arena.size, bool), np.zeros(vad_arena.size, bool)
    for i, x in enumerate(files):
        F = x.shape[0] // FRAME
        _, _, oo, vo = table[i]
        no, nv = max(F - 1, 0) * FRAME * channels, F * channels
        outs.append(out_arena[oo:oo + no].reshape(-1, channels).copy())
        vads.append(vad_arena[vo:vo + nv].reshape(-1, channels).copy())
        seen_out[oo:oo + no] = True
        seen_vad[vo:vo + nv] = True
    assert (out_arena[~seen_out] == (CANARY_I16 if out_i16 else CANARY_F32)).all(), "a byte outside the files' output ranges was written"
    assert (vad_arena[~seen_vad] == CANARY_F32).all(), "a VAD value outside the files' ranges was written"
    return outs, vads, s, want_in


def assert_files_equal(outs, vads, files, channels, want, what=""):
    """Every file's audio and VAD against want(i) -> (audio, vad): counts (F - 1) * 480 and F, then every bit."""
    for i, x in enumerate(files):
        F = x.shape[0] // FRAME
        wo, wv = want(i)
        assert outs[i].shape == (max(F - 1, 0) * FRAME, channels) and vads[i].shape == (F, channels), (what, i, outs[i].shape, vads[i].shape)
        assert outs[i].shape == wo.shape and vads[i].shape == wv.shape, (what, i)
        assert np.array_equal(bits(outs[i]), bits(wo)), (what, i, F)
        assert np.array_equal(bits(vads[i]), bits(wv)), (what, i, F)


def plan_restated(n_slots, step, frames):
    """The plan rule of include/nnn_pack.h in ten lines: (slot_of_file, first_step_of_file, steps, per-file padding)."""
    slot_of, first_of, pad_of = [-1] * len(frames), [-1] * len(frames), [0] * len(frames)
    rem, cur, queue, steps = [0] * n_slots, [-1] * n_slots, [i for i, F in enumerate(frames) if F > 0], []
    while True:
        for g in range(n_slots):
            if rem[g] == 0 and queue:
                cur[g] = queue.pop(0)
                rem[g], slot_of[cur[g]], first_of[cur[g]] = frames[cur[g]], g, len(steps)
        if max(rem) == 0:
            return slot_of, first_of, steps, pad_of
        n_k = min(step, max(rem))
        for g in range(n_slots):
            if rem[g] > 0:
                used = min(rem[g], n_k)
                pad_of[cur[g]] += n_k - used
                rem[g] -= used
        steps.append(n_k)
