"""python -m nnnoiseless_amd.files --out-dir D a.wav b.wav ...: the reference CLI (src/nnnoiseless.rs:230-334) over many files at once.

Every input is a 48 kHz WAV of 16-, 24- or 32-bit integers or 32-bit floats, any channel count; every output is a 48 kHz 16-bit WAV of the
same name in D with the same channels, holding what the CLI writes for that file: whole frames only, the first one dropped.  The files of
one channel count and sample format go through a batch in ONE packer run (pcm.denoise_files, include/nnn_pack.h), longest first: a corpus
of 16-bit mono files is one run.  The samples are converted on the GPU, by the packer's input kernel; the host only finds the `data` chunk.
"""
import argparse
import os
import struct
import sys

import numpy as np

from . import pcm

_KSDATAFORMAT_TAIL = bytes.fromhex("000000001000800000aa00389b71")   # bytes 2..15 of the PCM / IEEE-float subformat GUIDs


def read_wav(path):
    """A minimal RIFF reader: the `fmt ` and `data` chunks, format tags 1 (integer PCM) and 3 (IEEE float), and WAVE_FORMAT_EXTENSIBLE
    with those two subformats.  Returns (packer input format, channels, sample rate, data): data is int16 [n, channels] for 16-bit,
    uint8 [n * channels * 3] for packed 24-bit, int32 / float32 [n, channels] for 32-bit -- the file's bytes, not converted."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 12 or raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
        raise SystemExit(f"{path}: not a RIFF/WAVE file")
    fmt = data = None
    pos = 12
    while pos + 8 <= len(raw):
        tag, size = raw[pos:pos + 4], struct.unpack_from("<I", raw, pos + 4)[0]
        body = raw[pos + 8:pos + 8 + size]
        if tag == b"fmt " and fmt is None:
            fmt = body
        elif tag == b"data" and data is None:
            data = body   # (a size that runs past the end of the file -- a recording cut short -- yields what is there)
        pos += 8 + size + (size & 1)
    if fmt is None or len(fmt) < 16 or data is None:
        raise SystemExit(f"{path}: no fmt or data chunk")
    tag, channels, rate, _, align, bits = struct.unpack_from("<HHIIHH", fmt, 0)
    if tag == 0xFFFE:
        if len(fmt) < 40 or fmt[26:40] != _KSDATAFORMAT_TAIL:
            raise SystemExit(f"{path}: WAVE_FORMAT_EXTENSIBLE with a subformat that is neither PCM nor IEEE float")
        tag = struct.unpack_from("<H", fmt, 24)[0]
    if tag not in (1, 3) or channels < 1:
        raise SystemExit(f"{path}: format tag {tag} (integer PCM and IEEE float are read)")
    if rate != 48000:
        raise SystemExit(f"{path}: {rate} Hz; the packer takes 48 kHz files only -- resample first (pcm.Resampler brings any rate to 48 kHz on the GPU)")
    if tag == 1 and bits == 8:
        raise SystemExit(f"{path}: 8-bit samples are not read; convert to 16-bit (and see pcm.Resampler for other rates)")
    if (tag, bits) not in ((1, 16), (1, 24), (1, 32), (3, 32)) or align != channels * bits // 8:
        raise SystemExit(f"{path}: {bits}-bit samples of format tag {tag} are not read (16-, 24-, 32-bit integers and 32-bit floats are)")
    n = len(data) // align
    a = np.frombuffer(data, np.uint8, n * align)
    if bits == 16:
        return pcm.PCM_I16, channels, rate, a.view("<i2").reshape(n, channels)
    if bits == 24:
        return pcm.PACK_I24, channels, rate, a
    if tag == 1:
        return pcm.PACK_I32, channels, rate, a.view("<i4").reshape(n, channels)
    return pcm.PACK_F32_WAV, channels, rate, a.view("<f4").reshape(n, channels)


def write_wav16(path, x, channels):
    """x: int16 [n, channels] -> a 48 kHz 16-bit WAV, as the CLI's writer makes it."""
    body = np.ascontiguousarray(x, dtype="<i2").tobytes()
    head = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(body), b"WAVE", b"fmt ", 16, 1, channels, 48000, 48000 * channels * 2, channels * 2,
                       16, b"data", len(body))
    with open(path, "wb") as f:
        f.write(head + body)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nnnoiseless_amd.files", description="Denoise many 48 kHz WAV files in one batch.")
    ap.add_argument("--out-dir", required=True, help="where the denoised 16-bit WAVs go, under their inputs' names")
    ap.add_argument("--streams", type=int, default=None, help="streams of the batch (default: one slot per file, 4096 streams at the most)")
    ap.add_argument("--model", default=None, help="path to a custom .rnn model file")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("inputs", nargs="+")
    args = ap.parse_args(argv)
    names = [os.path.basename(p) for p in args.inputs]
    if len(set(names)) != len(names):
        raise SystemExit("two inputs share a file name: their outputs would overwrite each other")
    model = None
    if args.model:
        from . import RnnModel
        model = RnnModel.from_bytes(open(args.model, "rb").read())
    runs = {}   # (channels, format) -> [(name, data)]
    for path, name in zip(args.inputs, names):
        fmt, channels, _, data = read_wav(path)
        runs.setdefault((channels, fmt), []).append((name, data))
    os.makedirs(args.out_dir, exist_ok=True)
    for (channels, fmt), group in sorted(runs.items()):
        n_streams = None
        if args.streams is not None:
            n_streams = max(channels, args.streams - args.streams % channels)
        outs, _, s = pcm.denoise_files([d for _, d in group], channels, model, n_streams, "longest_first", fmt, pcm.PCM_I16, args.device)
        for (name, _), o in zip(group, outs):
            write_wav16(os.path.join(args.out_dir, name), o, channels)
        print(f"{len(group)} files of {channels} channel(s): {s['steps']} steps, {s['useful']} useful and {s['padded']} padded stream-frames, "
              f"{s['held_frames']} held", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
