"""The host layer's Radiance .hdr decoder against the REFERENCE's own loader: random files -- flat and run-length
coded scanlines, header variants, truncated bodies -- against what the reference's inc/hdr_loader.h (built behind a
harness as oracle/_ref/libref_hdr.so by `make -C oracle ref`) returned for the same files, recorded in
tests/golden/reference_outputs.json by oracle/gen_reference_outputs.py.  The committed fixtures of
test_hdr_golden.py cover hand-made files of the same decoder."""
import hashlib
import json
import os

import numpy as np
import pytest

from volumerenderercl_amd import datraw

HERE = os.path.dirname(os.path.abspath(__file__))


def recorded(case):
    """What the reference returned for `case` (read when a test runs: oracle/gen_reference_outputs.py imports this
    module to write the file)."""
    with open(os.path.join(HERE, "golden", "reference_outputs.json")) as f:
        return json.load(f)["hdr_random"][case]


def _rle_row(row, rng):
    """One run-length coded scanline (new RLE): marker 2 2 hi lo, then the 4 component planes as run / literal
    packets whose lengths a coin decides (any valid packet sequence decodes to the same row)."""
    w = row.shape[0]
    out = bytearray([2, 2, w >> 8, w & 255])
    for c in range(4):
        plane = row[:, c]
        i = 0
        while i < w:
            run = 1
            while i + run < w and run < 127 and plane[i + run] == plane[i]:
                run += 1
            if run >= 2 and rng.random() < 0.7:
                run = int(rng.integers(2, run + 1)) if run > 2 else run
                out += bytes([128 + run, int(plane[i])])
                i += run
            else:
                n = int(rng.integers(1, min(128, w - i) + 1))
                out += bytes([n]) + bytes(int(v) for v in plane[i:i + n])
                i += n
    return bytes(out)


def write_case(case, d):
    """The random .hdr file of `case`, written into directory d; returns its path."""
    rng = np.random.default_rng(66261004 + case)
    w, h = int(rng.integers(1, 70)), int(rng.integers(1, 12))
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    px[..., 3] = rng.integers(100, 150, (h, w))
    if rng.random() < 0.6:   # long runs, so that run packets appear
        rep = int(rng.integers(2, 9))
        px = np.repeat(px[:, ::rep], rep, axis=1)[:, :w]
    if rng.random() < 0.5:
        px[int(rng.integers(h)), int(rng.integers(w)), 3] = 0   # exponent 0 = black
    rle = 8 <= w < 32768 and rng.random() < 0.6
    if not rle and w >= 8:
        px[:, 0, 0] = 7        # a flat scanline must not start like the run-length marker
    body = b"".join(_rle_row(r, rng) for r in px) if rle else px.tobytes()
    magic = str(rng.choice(["#?RADIANCE", "#?RGBE"]))
    header = magic + "\n"
    if rng.random() < 0.5:
        header += "# a comment\n"
    header += "FORMAT=32-bit_rle_%s\n" % str(rng.choice(["rgbe", "xyze"]))
    if rng.random() < 0.4:
        header += "EXPOSURE=%g\n" % float(rng.choice([0.5, 1.0, 2.0]))
    header += "\n-Y %d +X %d\n" % (h, w)
    if rng.random() < 0.15:
        body = body[:int(len(body) * rng.uniform(0.2, 0.9))]   # truncated file
    path = os.path.join(d, "r.hdr")
    with open(path, "wb") as f:
        f.write(header.encode() + body)
    return path


@pytest.mark.parametrize("case", range(48))
def test_random_hdr_files_decode_like_the_reference(case, tmp_path):
    path = write_case(case, str(tmp_path))
    want = recorded(case)
    with open(path, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == want["input_sha256"], "the recorded file was another"
    if not want["ok"]:
        with pytest.raises(RuntimeError, match="Error loading environment map file."):
            datraw.load_hdr(path)
        return
    got = datraw.load_hdr(path)
    assert got.shape == tuple(want["shape"]) and got.dtype == np.float32
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == want["pixels_sha256"]   # bit-exact
