"""The device copies of the fp32 building blocks against the oracle, bit for bit, at chosen arguments.

tests/hip/probe_math.hip includes vr_device_math.h and vr_sampling.h unchanged and is compiled here with exactly
the product's numerics flags (`make print-hipflags` in csrc).  It evaluates every operation on every point of
tests/math_argsets.py on the GPU; the result bits must equal those of the oracle's batch entry
(vro.math_batch).  The only licence: a NaN equals a NaN of any payload.  No point is left out.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle import vro
from tests import math_argsets as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "volumerenderercl_amd", "csrc")
PROBE_SRC = os.path.join(ROOT, "tests", "hip", "probe_math.hip")
MAGIC = 0x4d525056
NO_TABLE = 0xffffffff


def product_hipflags():
    return subprocess.check_output(["make", "-s", "--no-print-directory", "-C", CSRC, "print-hipflags"],
                                   text=True).split()


def build_probe(out_dir, flags=None, include=CSRC):
    exe = os.path.join(str(out_dir), "probe_math")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + (product_hipflags() if flags is None else flags) +
                          ["-I", include, PROBE_SRC, "-o", exe])
    return exe


def write_request(path, cases, tables):
    with open(path, "wb") as f:
        np.array([MAGIC, len(tables), len(cases)], dtype=np.uint32).tofile(f)
        for tff, prefix in tables:
            np.array([len(tff), len(prefix)], dtype=np.uint32).tofile(f)
            np.ascontiguousarray(tff, dtype=np.uint8).tofile(f)
            np.ascontiguousarray(prefix, dtype=np.uint32).tofile(f)
        for op, _, args, ti in cases:
            np.array([vro.MATH_OP_ID[op], len(args), NO_TABLE if ti is None else ti], dtype=np.uint32).tofile(f)
            args.tofile(f)


def run_probe(exe, cases, tables, work_dir):
    """One fresh child process for all records; returns the result bits per case."""
    req, res = os.path.join(str(work_dir), "request.bin"), os.path.join(str(work_dir), "result.bin")
    write_request(req, cases, tables)
    p = subprocess.run(["timeout", "-k", "10", "60", exe, req, res], capture_output=True, text=True)
    assert p.returncode == 0, "probe_math ended with status %d: %s" % (p.returncode, p.stderr[-2000:])
    words = np.fromfile(res, dtype=np.uint32)
    assert words[0] == MAGIC
    out, pos = [], 1
    for op, _, args, _ in cases:
        n = len(args) * vro.math_arity(op)[1]
        out.append(words[pos:pos + n].reshape(len(args), -1))
        pos += n
    assert pos == words.size
    return out


def mismatches(dev, ref):
    """rows whose bits differ, a NaN on both sides counting as equal"""
    nan = lambda u: (u & 0x7fffffff) > 0x7f800000   # noqa: E731
    return np.nonzero(((dev != ref) & ~(nan(dev) & nan(ref))).any(axis=1))[0]


def oracle_results(cases, tables):
    out = []
    for op, _, args, ti in cases:
        tff, prefix = tables[ti] if ti is not None else (None, None)
        out.append(vro.math_batch(op, args, tff=tff, prefix=prefix))
    return out


def compare(cases, dev, ref):
    """{op: (points, mismatching points, first few mismatches as text)}"""
    report = {}
    for (op, tag, args, ti), d, r in zip(cases, dev, ref):
        bad = mismatches(d, r)
        n, nb, txt = report.get(op, (0, 0, []))
        for i in bad[:3]:
            txt.append("%s[%s, table %s] args %s: device %s, oracle %s" % (
                op, tag, ti, ["%08x" % v for v in args[i]], ["%08x" % v for v in d[i]], ["%08x" % v for v in r[i]]))
        report[op] = (n + len(args), nb + len(bad), txt)
    return report


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """Build the probe, run it once on every case, compare with the oracle: once for the module.  When the
    probe fails, the module fails here and nothing more runs on the GPU."""
    work = tmp_path_factory.mktemp("probe_math")
    exe = build_probe(work)
    cases, tables = list(A.cases()), A.tables()
    ref = oracle_results(cases, tables)
    dev = run_probe(exe, cases, tables, work)
    for (op, _, args, ti), d in zip(cases, dev):
        if op == "skip_test" and len(tables[ti][0]) >= 3:
            assert set(np.unique(d)) == {0, 1}, "skip_test must take both outcomes on table %d" % ti
    return compare(cases, dev, ref)


def test_every_operation_is_probed(report):
    assert set(report) == set(vro.MATH_OPS)


@pytest.mark.parametrize("op", vro.MATH_OPS)
def test_device_equals_oracle(report, op):
    points, bad, txt = report[op]
    print("%s: %d points, %d differ" % (op, points, bad))
    assert bad == 0, "%d of %d points differ:\n%s" % (bad, points, "\n".join(txt))
