"""The C++ host loader against the REFERENCE's own DatRawReader: random .dat/.raw files against what the reference's
src/io/datrawreader.cpp (built as oracle/_ref/libref_datraw.so by `make -C oracle ref`) read from the same files,
recorded in tests/golden/reference_outputs.json by oracle/gen_reference_outputs.py.  The committed fixtures of
test_loader_golden.py cover hand-made files of the same reader."""
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
        return json.load(f)["loader_random"][case]


def _random_dataset(rng, d):
    """Writes a .dat with its .raw file(s) into d; returns the .dat's path."""
    fmt = ["UCHAR", "USHORT", "FLOAT"][int(rng.integers(3))]
    res = [int(v) for v in rng.integers(1, 9, size=3)]
    n = res[0] * res[1] * res[2]
    big = fmt != "UCHAR" and rng.random() < 0.4
    steps = int(rng.choice([1, 1, 1, 2, 3]))
    sep = str(rng.choice([" ", "\t", "  ", " \t"]))
    names = []
    for t in range(steps):
        name = "v%d_%d.raw" % (int(rng.integers(1000)), t)
        if fmt == "UCHAR":
            a = rng.integers(0, int(rng.choice([2, 17, 256])), n).astype(np.uint8)
        elif fmt == "USHORT":
            a = rng.integers(0, int(rng.choice([2, 300, 4096, 65536])), n).astype(">u2" if big else "<u2")
        else:
            a = (rng.random(n) * float(rng.choice([0.5, 1.0, 7.5, 1000.0]))).astype(">f4" if big else "<f4")
            if rng.random() < 0.2:
                a[:] = 0      # an all-zero field: what does the normalisation divide by?
        a.tofile(os.path.join(d, name))
        names.append(name)
    lines = ["ObjectFileName:%s%s" % (sep, " ".join(names))]
    cube = res[0] == res[1] == res[2] and rng.random() < 0.5 and steps == 1
    if not cube:
        lines.append("Resolution:%s%d %d %d" % (sep, res[0], res[1], res[2]))
    lines.append("Format:%s%s" % (sep, fmt))
    if rng.random() < 0.6:
        th = [float(rng.choice([0.5, 1.0, 1.0, 2.5, 3.0])) for _ in range(3)]
        lines.append("SliceThickness:%s%g %g %g" % (sep, th[0], th[1], th[2]))
    if big or rng.random() < 0.2:
        lines.append("Endianness:%s%s" % (sep, "BIG" if big else "LITTLE"))
    if rng.random() < 0.3:
        lines.append("ObjectModel:%sI" % sep)
    if rng.random() < 0.3:
        lines.append("Unknown:%swhatever 1 2 3" % sep)
    order = rng.permutation(len(lines) - 1) + 1 if rng.random() < 0.5 else np.arange(1, len(lines))
    lines = [lines[0]] + [lines[i] for i in order]
    dat = os.path.join(d, "f.dat")
    with open(dat, "w") as f:
        f.write("\n".join(lines) + ("\n" if rng.random() < 0.8 else ""))
    return dat


def write_case(case, d):
    """The random data set of `case`, written into directory d; returns the .dat's path."""
    return _random_dataset(np.random.default_rng(44261004 + case), d)


def input_sha256(d):
    """One hash over every file of the data set (names and bytes, in name order)."""
    h = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()


@pytest.mark.parametrize("case", range(64))
def test_random_files_read_like_the_reference(case, tmp_path):
    dat = write_case(case, str(tmp_path))
    want = recorded(case)
    assert input_sha256(str(tmp_path)) == want["input_sha256"], "the recorded data set was another"
    r = datraw.DatRawReader()
    if want["rc"] != 0:
        with pytest.raises(RuntimeError) as e:
            r.read_files(datraw.Properties(dat))
        assert str(e.value) == want["error"]
        return
    r.read_files(datraw.Properties(dat))
    p = r.properties()
    assert p.volume_res == want["res"]
    assert p.slice_thickness == want["thickness"]
    assert p.format == want["format"] and p.endianness == want["endianness"]
    assert p.image_channel_order == want["channel_order"]
    assert len(r.data()) == want["n_timesteps"]
    # NaN == NaN here: an all-zero FLOAT field divides 0 by 0 in both readers
    np.testing.assert_array_equal(np.float32([p.min_value, p.max_value]), np.float32(want["min_max"]))
    for t in range(want["n_timesteps"]):
        assert hashlib.sha256(r.data()[t].tobytes()).hexdigest() == want["data_sha256"][t], "time step %d" % t   # bit-exact
        hist = np.ascontiguousarray(r.histograms()[t], dtype=np.float64)
        assert hashlib.sha256(hist.tobytes()).hexdigest() == want["histogram_sha256"][t], "histogram %d" % t
