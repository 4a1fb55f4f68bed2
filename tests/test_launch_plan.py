"""The launch plan (csrc/ba3c_plan.h: which kernels share a launch, which stream, which geometry,
how many partial slabs) on the host: tests/plan_table.cpp is compiled with the host c++ and asked
for the plan at points read off the launch code before the plan existed (256 CUs), for what each
single switch value changes, and for the invariants over every batch, CU count, channel count
and switch combination.  The same program built with -fsanitize=address,undefined answers the
same points (and every 7th batch of the invariants: it is five times slower)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "plan_table.cpp")
INC = os.path.join(ROOT, "distributed-ba3c_amd", "csrc")

# the order of plan_table's switch values, and the defaults
SWITCHES = ["generic", "c1pair", "scalars_ride", "overlap", "multi", "multi_big", "fused_update", "ring",
            "chain", "fwd01"]
DEFAULT = dict(generic=0, c1pair=2, scalars_ride=1, overlap=2, multi=1, multi_big=3, fused_update=1, ring=1,
               chain=1, fwd01=1)
BATCHES = [32, 128, 129, 160, 512, 513, 1024, 1280, 2048, 4100]


@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    cxx = shutil.which("c++")
    assert cxx, "the host compiler c++ is required"
    out = tmp_path_factory.mktemp("plan_table")
    built = {}
    for name, flags in (("plain", ["-O3"]),
                        ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(out / ("plan_table_" + name))
        subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC, SRC, "-o", exe],
                       check=True)
        built[name] = exe
    return built


def plans(exe, queries):
    """queries: (B, C, cus, train, {switch: value}) -> one dict per query."""
    args = []
    for B, C, cus, train, sw in queries:
        s = dict(DEFAULT, **sw)
        args.append("%d:%d:%d:%d:%s" % (B, C, cus, train, ",".join(str(s[k]) for k in SWITCHES)))
    out = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(queries)
    rows = []
    for line in out:
        row = dict(kv.split("=") for kv in line.split())
        rows.append({k: (v if k == "conv1_wgrad" else int(v)) for k, v in row.items()})
    return rows


def plan(exe, B, C=4, cus=256, train=1, **sw):
    return plans(exe, [(B, C, cus, train, sw)])[0]


@pytest.mark.parametrize("build", ["plain", "san"])
def test_default_plan_at_256_cus(binaries, build):
    exe = binaries[build]
    for B in (32, 128):
        p = plan(exe, B)
        assert p["prep_multi"] and p["mj"] and p["mj_fc"] and not p["fc1_big_tiles"] and not p["mj_c2"], B
        assert p["conv2_small"] and not p["side_stream"] and not p["big"], B
        assert p["conv1_wgrad"] == "wgrad6" and p["conv1_slabs"] == max(64, min(256, 3 * B)), B
        assert not p["ring_fwd"] and not p["fwd01"] and not p["ring_dgrad"], B
    for B in (129, 160):
        p = plan(exe, B)
        assert not p["prep_multi"] and not p["mj"], B
        assert p["mj_fc"] and p["fc1_big_tiles"] and p["mj_c2"] and p["big"], B
        assert not p["conv2_small"] and not p["side_stream"], B
        assert p["conv1_wgrad"] == "wgrad6" and p["conv1_slabs"] == 256, B
    p = plan(exe, 512)
    assert p["ring_fwd"] and p["ring_dgrad"] and p["fwd01"]
    assert p["conv1_wgrad"] == "whole" and p["conv1_slabs"] == 512
    p = plan(exe, 513)
    assert not p["ring_fwd"] and not p["ring_dgrad"] and not p["fwd01"]
    assert p["conv1_wgrad"] == "whole" and p["conv1_slabs"] == 512
    for B in (1024, 2048):
        p = plan(exe, B)
        assert p["ring_fwd"] and p["ring_dgrad"] and p["fwd01"], B
        assert p["conv1_wgrad"] == "pair0" and p["conv1_slabs"] == 256 and p["conv0_slabs"] == 256, B
    p = plan(exe, 1280)   # the pair follows the switch and the geometry, not the ring walk
    assert p["conv1_wgrad"] == "pair0" and p["conv1_slabs"] == 256 and p["conv0_slabs"] == 256
    assert not p["ring_fwd"] and not p["ring_dgrad"] and not p["fwd01"]
    p = plan(exe, 4100)
    assert p["ring_fwd"] and p["ring_dgrad"] and p["fwd01"]
    assert p["conv1_wgrad"] == "whole" and p["conv1_slabs"] == 512 and p["conv0_slabs"] == 512
    # conv0: 10 bands per image up to 512 slabs; conv3: one slab per image up to one per CU
    assert [plan(exe, B)["conv0_slabs"] for B in (1, 32, 51, 52, 160)] == [10, 320, 510, 512, 512]
    assert [plan(exe, B)["conv3_slabs"] for B in (1, 32, 255, 256, 2048)] == [1, 32, 255, 256, 256]
    assert [plan(exe, B, cus=304)["conv3_slabs"] for B in (255, 300, 2048)] == [255, 256, 256]
    assert [plan(exe, B)["conv1_slabs"] for B in (1, 7, 8, 21, 22, 85, 86, 511)] == [9, 63, 64, 64, 66, 255, 256, 256]


@pytest.mark.parametrize("build", ["plain", "san"])
def test_twelve_channels_and_generic_engine(binaries, build):
    exe = binaries[build]
    for B in BATCHES:
        p = plan(exe, B, C=12)
        assert not (p["prep_multi"] or p["mj"] or p["mj_fc"] or p["fc1_big_tiles"] or p["mj_c2"] or p["fwd01"]), B
        assert p["conv1_wgrad"] != "pair0" and p["conv0_slabs"] == 0, B
        assert p["side_stream"] == (B <= 128), B
        # conv1's band kernels do not depend on conv0's channels: ring walks and slabs as for C == 4
        q = plan(exe, B)
        assert (p["ring_fwd"], p["ring_dgrad"], p["conv1_slabs"], p["conv3_slabs"]) == \
               (q["ring_fwd"], q["ring_dgrad"], q["conv1_slabs"], q["conv3_slabs"]), B
        assert p["conv1_wgrad"] == ("whole" if B >= 512 else "wgrad6"), B
        for C in (4, 12):
            g = plan(exe, B, C=C, generic=1)
            assert not g["split"] and g["conv1_wgrad"] == "gemm", (B, C)
            assert not any(g[k] for k in ("prep_multi", "ring_fwd", "fwd01", "conv2_small", "mj", "mj_fc",
                                          "fc1_big_tiles", "mj_c2", "ring_dgrad")), (B, C)
            assert g["side_stream"] == (B <= 128), (B, C)
    # an inference plan: the same forward, no backward decision
    for B in BATCHES:
        t, f = plan(exe, B), plan(exe, B, train=0)
        for k in ("split", "prep_multi", "ring_fwd", "fwd01", "conv2_small"):
            assert f[k] == t[k], (B, k)
        assert not any(f[k] for k in ("big", "mj", "mj_fc", "fc1_big_tiles", "mj_c2", "side_stream", "ring_dgrad")), B


# what each single non-default value changes at C == 4 and 256 CUs, as its comment in Switches says:
# field -> (batches at which it differs from the default plan, its value there)
SMALL, BIG = [32, 128], [129, 160, 512, 513, 1024, 1280, 2048, 4100]
RING_B, PAIR_B = [512, 1024, 2048, 4100], [1024, 1280, 2048]
FLIPS = {
    ("generic", 1): {"split": (BATCHES, 0), "prep_multi": (SMALL, 0), "conv2_small": (SMALL, 0), "mj": (SMALL, 0),
                     "mj_fc": (BATCHES, 0), "fc1_big_tiles": (BIG, 0), "mj_c2": (BIG, 0), "side_stream": (SMALL, 1),
                     "ring_fwd": (RING_B, 0), "fwd01": (RING_B, 0), "ring_dgrad": (RING_B, 0),
                     "conv1_wgrad": (BATCHES, "gemm")},
    ("c1pair", 0): {"conv1_wgrad": (PAIR_B, "whole")},
    ("scalars_ride", 0): {},
    ("overlap", 0): {},
    ("overlap", 1): {"mj": (SMALL, 0), "mj_fc": (BATCHES, 0), "fc1_big_tiles": (BIG, 0), "mj_c2": (BIG, 0),
                     "side_stream": (BATCHES, 1)},
    ("multi", 0): {"prep_multi": (SMALL, 0), "mj": (SMALL, 0), "mj_fc": (BATCHES, 0), "fc1_big_tiles": (BIG, 0),
                   "mj_c2": (BIG, 0), "side_stream": (SMALL, 1)},
    ("multi_big", 0): {"mj_fc": (BIG, 0), "fc1_big_tiles": (BIG, 0), "mj_c2": (BIG, 0)},
    ("multi_big", 1): {"mj_c2": (BIG, 0)},
    ("multi_big", 2): {"mj_fc": (BIG, 0), "fc1_big_tiles": (BIG, 0)},
    ("fused_update", 0): {},
    ("ring", 0): {"ring_fwd": (RING_B, 0), "fwd01": (RING_B, 0), "ring_dgrad": (RING_B, 0),
                  "conv1_wgrad": (PAIR_B, "whole")},
    ("chain", 0): {},
    ("fwd01", 0): {"fwd01": (RING_B, 0)},
}


@pytest.mark.parametrize("build", ["plain", "san"])
def test_each_switch_flips_what_its_comment_names(binaries, build):
    exe = binaries[build]
    base = plans(exe, [(B, 4, 256, 1, {}) for B in BATCHES])
    for (name, value), flips in FLIPS.items():
        got = plans(exe, [(B, 4, 256, 1, {name: value}) for B in BATCHES])
        for B, d, g in zip(BATCHES, base, got):
            for k in d:
                where, to = flips.get(k, ([], None))
                if B in where:
                    assert g[k] == to and d[k] != to, (name, value, B, k, g[k], d[k])
                else:
                    assert g[k] == d[k], (name, value, B, k, g[k], d[k])
    # the side stream of the twelve-channel small batches is BA3C_OVERLAP's default
    assert [plan(exe, 32, C=12, overlap=v)["side_stream"] for v in (0, 1, 2)] == [0, 1, 1]
    assert [plan(exe, 160, C=12, overlap=v)["side_stream"] for v in (0, 1, 2)] == [0, 1, 0]


def test_invariants_over_every_batch_and_switch_combination(binaries):
    r = subprocess.run([binaries["plain"], "invariants"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("invariants ok"), r.stdout + r.stderr
    assert int(r.stdout.split()[2]) == 16384 * 3 * 2 * 3072
    r = subprocess.run([binaries["san"], "invariants-sparse"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("invariants ok"), r.stdout + r.stderr
