"""vrhip_render --preint without a device: what it composes with and what it is refused with, through the parser and
validate (csrc/host/vrhip_cli.cpp) in the stand-alone program of tests/test_cli_args.py (tests/cxx/cli_args_main.cpp,
built the same way).  --ranks is REFUSED with --preint, as with technique 6's options: the C++ tile gather is not
wired for it."""
import pytest

from tests.test_cli_args import AX, MESH, OUT, RAMP, STATS, _run, exe   # noqa: F401  (exe: the module's fixture)

PRE = OUT + ["--preint"]

ACCEPTED = [PRE, PRE + ["--orbit", "0", "1", "0", "8", "--frames-per-launch", "4", "--rgba8"],
            PRE + ["--camera-path", "p", "--frames-per-launch", "2"], PRE + ["--tf", "t.tff", "--illum", "0", "--rate", "0.5"],
            PRE + ["--no-ess", "--nearest", "--ortho", "--independent", "--frames", "3"]]

REFUSED = [PRE + a for a in (["--mip"], ["--iso", "0.5"], RAMP, ["--tf2d", "t.rgba", "8", "8", "0.25"], ["--pathtrace"], ["--ao"],
                             ["--show-ess"], ["--img-ess"], ["--env", "e.hdr"], ["--ranks", "2"], AX, ["--depth", "max"])]
REFUSED += [MESH + ["--preint"], STATS + ["--preint"]]


def test_preint_composes(exe):   # noqa: F811
    for args in ACCEPTED:
        res = _run(exe, args)
        assert res.returncode == 0 and res.stderr == "" and res.stdout.startswith("accepted: size "), (args, res.stderr[-2000:])


def test_preint_refusals_end_with_the_usage_text(exe):   # noqa: F811
    for args in REFUSED:
        res = _run(exe, args)
        assert res.returncode == 2 and res.stderr.startswith("usage: vrhip_render (--dat FILE.dat | --synth") and \
            res.stdout == "", (args, res.stderr[-2000:])
    assert "[--preint]" in _run(exe, ["--help"]).stderr
