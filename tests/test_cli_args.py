"""vrhip_render's options without a device: the parser and the refusals (csrc/host/vrhip_cli.cpp) are compiled here --
not loaded into python -- with AddressSanitizer and UBSan into a stand-alone program with its own main
(tests/cxx/cli_args_main.cpp), which is run once per argument vector in the environment as it is.  What is refused
ends with the usage text (or the option's own message) and status 2, what is accepted reaches the end."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "volumerenderercl_amd", "csrc", "host")

SCENE = ["--synth", "shells", "32", "UCHAR"]
OUT = SCENE + ["--out", "x"]
AX = ["--slice-axis", "Z", "0"]
PLANE = ["--slice", "0", "0", "0", "1", "0", "0", "0", "1", "0"]
RAMP = ["--tf2d-ramp", "8", "0.25", "0.0", "0.1"]
MESH = SCENE + ["--mesh", "0.5", "m.ply"]
STATS = SCENE + ["--stats", "s.json"]

# every vector ends with the usage text and status 2
REFUSED = [[], ["--help"], ["--no-such-option"], SCENE, ["--out", "x"]]
# a missing argument, one or two per option group
REFUSED += [["--dat"], ["--synth", "sphere", "32"], ["--size", "40"], ["--orbit", "0", "1", "0"], ["--bg", "1", "1"], ["--iso"],
            ["--tf2d", "t.rgba", "8", "8"], ["--slab", "0.1", "4"], ["--depth", "iso"], ["--mesh", "0.5"], ["--stats-bins", "8"],
            ["--filter", "gauss"], ["--frames-per-launch"], ["--tile"], ["--out"], ["--dump-views"]]
# technique 2 and 4
REFUSED += [OUT + a for a in (["--mip", "--pathtrace"], ["--iso-refine", "3"])]
REFUSED += [OUT + ["--iso", "0.35"] + a for a in (["--mip"], ["--pathtrace"], ["--ao"], ["--show-ess"], ["--img-ess"], ["--env", "none.hdr"],
                                                   ["--iso-refine", "17"], ["--iso-refine", "-1"])]
# technique 6
REFUSED += [OUT + a for a in (["--tf2d-ramp", "8", "0.25", "0.1", "0.1"], ["--tf2d-ramp", "0", "0.25", "0.0", "0.1"],
                              ["--tf2d-ramp", "8", "0", "0.0", "0.1"], RAMP + ["--mip"], RAMP + ["--iso", "0.5"], RAMP + ["--ranks", "2"],
                              RAMP + ["--ao"], ["--tf2d", "t.rgba", "4097", "1", "0.25"], ["--tf2d", "t.rgba", "512", "129", "0.25"],
                              ["--tf2d", "t.rgba", "8", "8", "0.25"] + RAMP, ["--tf2d", "t.rgba", "8", "8", "nan"])]
# slice views
REFUSED += [OUT + a for a in (AX + ["--mip"], AX + ["--iso", "0.5"], AX + ["--pathtrace"], AX + ["--orbit", "0", "1", "0", "4"],
                              AX + ["--camera-path", "nowhere"], AX + ["--ranks", "2"], AX + PLANE, AX + RAMP, ["--slab", "0.1", "4", "max"],
                              ["--slice-stack", "4"], ["--slice-value"], ["--slice-axis", "Q", "0"], ["--slice-axis", "Z"],
                              AX + ["--slab", "0.1", "0", "max"], AX + ["--slab", "0.1", "257", "max"],
                              AX + ["--slab", "0.1", "4", "median"], AX + ["--slice-stack", "0"], PLANE[:-1],
                              ["--slice", "0", "0", "0", "0", "0", "0", "0", "1", "0", "--slab", "0.1", "2", "max"],
                              ["--slice", "0", "0", "0", "1", "0", "0", "2", "0", "0", "--slice-stack", "3"])]
# depth images
REFUSED += [OUT + ["--depth", "max"] + a for a in (["--pathtrace"], ["--mip"], ["--iso", "0.4"], AX, ["--slice-value"], ["--ranks", "2"],
                                                   ["--frames-per-launch", "4"], ["--orbit", "0", "1", "0", "4"],
                                                   ["--camera-path", "none"], ["--frames", "2"], ["--rgba8"], ["--img-ess"],
                                                   ["--size", "64", "48", "--depth-rect", "60", "0", "8", "8"], RAMP)]
REFUSED += [OUT + a for a in (["--depth", "min"], ["--depth", "iso", "0.4", "--depth-refine", "17"], ["--depth-refine", "3"],
                              ["--depth-rect", "0", "0", "4", "4"], ["--depth", "iso", "0.4", "--iso-refine", "3"])]
# meshes
REFUSED += [MESH + a for a in (["--pathtrace"], ["--mip"], ["--iso", "0.4"], AX, ["--depth", "max"], ["--ranks", "2"], ["--frames", "2"],
                               ["--rgba8"], ["--orbit", "0", "1", "0", "4"], ["--frames-per-launch", "4"], ["--img-ess"], ["--bench"],
                               ["--independent"], ["--downsample", "2"], ["--dump-tf", "t"], ["--timestep", "-1"],
                               ["--mesh-region", "0", "0", "0", "8", "8", "8193"])]
REFUSED += [SCENE + a for a in (["--mesh", "0.5", "out.obj"], ["--mesh", "0.5", "out"], ["--mesh-normals"],
                                ["--mesh-region", "0", "0", "0", "8", "8", "8"], ["--timestep", "1"], ["--mesh", "nan", "out.ply"],
                                ["--mesh", "0.5", "out.stl", "--mesh-indexed"], ["--mesh-indexed"], ["--out", "frame", "--mesh-indexed"])]
# statistics
REFUSED += [STATS + a for a in (["--pathtrace"], ["--mip"], ["--iso", "0.4"], AX, ["--depth", "max"], ["--mesh", "0.5", "m.ply"],
                                ["--ranks", "2"], ["--frames", "2"], ["--rgba8"], ["--stats-bins", "4096", "17"], ["--stats-bins", "0", "1"],
                                ["--stats-window", "0.5", "0.5", "1"], ["--stats-bins", "8", "2", "--stats-window", "0", "1", "0"],
                                ["--timestep", "-1"], ["--stats-region", "0", "0", "0", "8", "8", "-1"])]
REFUSED += [OUT + a for a in (["--stats-moments"], ["--stats-bins", "8", "2"], ["--stats-window", "0", "1", "1"], ["--stats-hist", "h.u64"],
                              ["--stats-region", "0", "0", "0", "8", "8", "8"])]
# filters, camera paths, launch sets, what is left
REFUSED += [OUT + a for a in (["--filter", "box"], ["--filter", "gauss", "-1"], ["--filter", "gauss", "1.5", "9"], ["--filter"],
                              ["--filter", "median", "--ranks", "2"], ["--filter", "median", "--downsample", "2"],
                              ["--camera-path", ""], ["--camera-path", "p", "--orbit", "0", "1", "0", "4"], ["--orbit", "0", "0", "0", "4"],
                              ["--orbit", "0", "1", "0", "0"], ["--dump-views", "v"], ["--samples-per-launch", "-1"],
                              ["--tf-easing", "bounce"])]

# every vector passes the parser and every refusal
ACCEPTED = [OUT, OUT + ["--size", "40", "24", "--rotate", "1", "1", "0", "30", "--translate", "0", "0", "2.5", "--bg", "0", "0", "0"],
            OUT + ["--view"] + ["1"] * 16 + ["--seed", "4294967295", "--illum", "0", "--no-ess", "--ortho", "--nearest"],
            OUT + ["--mip", "--orbit", "0", "1", "0", "8", "--frames-per-launch", "4", "--rgba8", "--bench"],
            OUT + ["--iso", "0.35", "--iso-refine", "16", "--ranks", "2", "--loopback", "--tile", "16", "--root-share", "0.5"],
            OUT + RAMP + ["--camera-path", "p", "--frames-in-flight", "3", "--round-budget", "32"],
            OUT + ["--tf2d", "t.rgba", "4096", "16", "0.25", "--tf-easing", "cubic", "--tf-stops", "s.tff"],
            OUT + ["--pathtrace", "--extinction", "50", "--frames", "8", "--samples-per-launch", "4", "--env", "e.hdr"],
            OUT + AX + ["--slab", "0.1", "256", "mean", "--slice-stack", "65536", "--slice-value", "--rgba8"],
            OUT + PLANE + ["--slice-stack", "3"],
            OUT + ["--size", "64", "48", "--depth", "opacity", "0.5", "--depth-rect", "30", "22", "13", "9", "--depth-refine", "0"],
            OUT + ["--depth", "max", "--filter", "gauss", "1.5", "3", "--filter", "median", "--filter", "gauss", "0.5"],
            MESH + ["--mesh-indexed", "--mesh-normals", "--mesh-region", "0", "0", "0", "30", "32", "17", "--timestep", "0"],
            SCENE + ["--mesh", "0.5", "dir.v2/m.stl", "--device-ingest"],
            STATS + ["--stats-bins", "4096", "16", "--stats-window", "0.1", "0.9", "0.5", "--stats-region", "3", "5", "2", "29", "30", "31",
                     "--stats-moments", "--stats-hist", "h.u64", "--timestep", "2", "--filter", "median"],
            ["--dat", "head.dat", "--downsample", "2"], OUT + ["--contours", "--aerial", "--ao", "--show-ess", "--img-ess", "--gradient-bg"],
            OUT + ["--state", "s.json", "--orbit", "0", "1", "0", "1048576", "--dump-views", "v.f32", "--device", "3", "--force-gather"]]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cli_args") / "cli_args_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                           os.path.join(HOST, "vrhip_cli.cpp"), os.path.join(ROOT, "tests", "cxx", "cli_args_main.cpp"), "-o", path])
    return path


def _run(exe, args):
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)


def test_refusals_end_with_the_usage_text(exe):
    for args in REFUSED:
        res = _run(exe, args)
        assert res.returncode == 2 and res.stderr.startswith("usage: vrhip_render (--dat FILE.dat | --synth") and \
            res.stderr.endswith("PREFIX.ppm and prints one JSON line\n") and res.stdout == "", (args, res.stderr[-2000:])


def test_refusals_with_a_message_of_their_own(exe, tmp_path):
    res = _run(exe, OUT + ["--rgba8", "--ranks", "2"])
    assert res.returncode == 2 and res.stderr.startswith("--rgba8 cannot be combined with --ranks: ") and res.stdout == ""
    taps = str(tmp_path / "taps.txt")
    for text in (None, "1\n1\n", "1\n1\n1\n1\n", "1 2 3 4 5 6 7 8 9 10\n1\n1\n", "1\nx\n1\n", "1\n\n1 inf\n1\n"):
        if text is not None:
            open(taps, "w").write(text)
        res = _run(exe, OUT + ["--filter", "taps", taps])
        assert res.returncode == 2 and res.stdout == "", text
        assert res.stderr == "--filter taps: %s does not hold three lines of 1 to 9 finite weights\n" % taps, text


def test_what_is_accepted_reaches_the_end(exe, tmp_path):
    taps = str(tmp_path / "taps.txt")
    open(taps, "w").write("# x, y, z\n0.5 0.25\n1\n 0.5 0.5 -0.25 0 0 0 0 0 0\n")
    for args in ACCEPTED + [OUT + ["--filter", "taps", taps]]:
        res = _run(exe, args)
        assert res.returncode == 0 and res.stderr == "" and res.stdout.startswith("accepted: size "), (args, res.stderr[-2000:])
    assert _run(exe, ACCEPTED[1]).stdout == "accepted: size 40 24 frames 1 filters 0\n"
    assert _run(exe, ACCEPTED[11]).stdout == "accepted: size 1024 1024 frames 1 filters 3\n"
