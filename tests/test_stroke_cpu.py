"""The host-only part of the stroke layer (include/dtp.h: dtp_stroke_plan; inpainter.plan_stroke): the C planner against the
independent pure-Python one of tests/stroke_ref.py on seeded random strokes, the edge cases of the disjointness rule by hand, the
header against the binding, and the planner's refusals.  No GPU."""
import ctypes as C
import os
import random
import re

import pytest

import stroke_ref
from stroke_ref import ERASE, INPAINT, OVERPAINT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 64


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def c_plan(lib, H, W, Rw, wrap, stamps, max_group):
    from diffusiontexturepainting_amd import _lib
    n = len(stamps)
    arr = (_lib.StrokeStamp * n)(*[_lib.StrokeStamp(x, y, m, 0, 0) for x, y, m in stamps])
    group_of, ng = (C.c_int * n)(), C.c_int(-1)
    rc = lib.dtp_stroke_plan(H, W, Rw, int(wrap), arr, n, max_group, group_of, C.byref(ng))
    assert rc == 0, lib.dtp_last_error()
    out = list(group_of)
    assert ng.value == out[-1] + 1
    return out


def random_stroke(rng, H, W, n, erase_at=()):
    """A stroke that moves by about a window at a time, so that disjoint and overlapping neighbours both occur; positions run past
    every border (the planner takes any int)."""
    x, y = rng.randrange(-R, W), rng.randrange(-R, H)
    out = []
    for i in range(n):
        x += rng.choice([-2 * R, -R - 1, -R, -R + 1, -R // 2, 0, R // 2, R - 1, R, R + 1, 2 * R, rng.randrange(-W, W)])
        y += rng.choice([0, 0, 0, -R, R, R - 1, rng.randrange(-H, H)])
        if not -2 * W <= x <= 3 * W:
            x = rng.randrange(0, W)
        if not -2 * H <= y <= 3 * H:
            y = rng.randrange(0, H)
        mode = ERASE if i in erase_at else rng.choice([INPAINT, INPAINT, OVERPAINT])
        out.append((x, y, mode))
    return out


# H != W; sizes that are no multiple of R; H < 2R: no pair of windows is disjoint on y under wrap (R <= d <= H - R is empty)
@pytest.mark.parametrize("H,W", [(96, 160), (200, 136), (64, 64), (127, 1000)])
@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("max_group", [1, 2, 8])
def test_planner_matches_the_independent_python_planner(lib, H, W, wrap, max_group):
    rng = random.Random(1000 * H + 10 * W + 2 * max_group + int(wrap))
    joined = 0
    for trial in range(12):
        stamps = random_stroke(rng, H, W, 24, erase_at=(7, 8, 15) if trial % 2 else ())
        got = c_plan(lib, H, W, R, wrap, stamps, max_group)
        assert got == stroke_ref.plan(H, W, R, wrap, stamps, max_group), (trial, stamps)
        assert got[0] == 0 and all(0 <= b - a <= 1 for a, b in zip(got, got[1:]))  # order kept: ids never decrease or skip
        joined += len(stamps) - (got[-1] + 1)
        for i in (7, 8, 15):
            if trial % 2:  # an Erase stamp is alone in its group
                assert got.count(got[i]) == 1
    if max_group == 1:
        assert joined == 0
    elif W >= 2 * R:
        assert joined > 0  # (the strokes do exercise the joining branch)


def test_hand_cases(lib):
    H, W = 96, 160
    for wrap in (False, True):
        assert c_plan(lib, H, W, R, wrap, [(0, 0, 0), (R, 0, 0)], 8) == [0, 0]        # d == R: edge to edge, disjoint
        assert c_plan(lib, H, W, R, wrap, [(0, 0, 0), (R - 1, 0, 0)], 8) == [0, 1]    # d == R - 1: one shared column
        assert c_plan(lib, H, W, R, wrap, [(R, 0, 0), (0, 0, 0)], 8) == [0, 0]        # ... in either order
        assert c_plan(lib, H, W, R, wrap, [(R - 1, 0, 0), (0, 0, 0)], 8) == [0, 1]
    # A window at x = W - R/2 wraps into columns 0 .. R/2 - 1.  The window at x = R/2 starts exactly where that ends (d == R, edge to
    # edge): disjoint with and without wrap.  One column to the left, at x = R/2 - 1, the two overlap -- only with wrap.
    pair = [(W - R // 2, 0, 0), (R // 2, 0, 0)]
    assert c_plan(lib, H, W, R, False, pair, 8) == [0, 0]
    assert c_plan(lib, H, W, R, True, pair, 8) == [0, 0]
    for first, second in ((W - R // 2, R // 2 - 1), (R // 2 - 1, W - R // 2), (W - R // 2, 0), (W - 1, 0)):
        pair = [(first, 0, 0), (second, 0, 0)]
        assert c_plan(lib, H, W, R, False, pair, 8) == [0, 0]
        assert c_plan(lib, H, W, R, True, pair, 8) == [0, 1]
    # wrap: d == L - R is still disjoint, d == L - R + 1 is not
    assert c_plan(lib, H, W, R, True, [(0, 0, 0), (W - R, 0, 0)], 8) == [0, 0]
    assert c_plan(lib, H, W, R, True, [(0, 0, 0), (W - R + 1, 0, 0)], 8) == [0, 1]
    # H < 2R: under wrap nothing is disjoint on y, without wrap rows 0 and 64 are (the second window hangs over the bottom edge)
    assert c_plan(lib, H, W, R, True, [(0, 0, 0), (0, R, 0)], 8) == [0, 1]
    assert c_plan(lib, H, W, R, False, [(0, 0, 0), (0, R, 0)], 8) == [0, 0]
    # coordinates far outside are reduced modulo the texture
    assert c_plan(lib, H, W, R, True, [(0, 0, 0), (R + 5 * W, -3 * H, 0)], 8) == [0, 0]
    assert c_plan(lib, H, W, R, True, [(0, 0, 0), (-W, 7 * H, 0)], 8) == [0, 1]
    # the order is kept: the third stamp would fit the FIRST group, but only the current one is open, and it overlaps that
    assert c_plan(lib, H, W, R, False, [(0, 0, 0), (10, 0, 0), (64, 0, 0)], 8) == [0, 1, 2]
    assert c_plan(lib, H, W, R, False, [(0, 0, 0), (10, 0, 0), (80, 0, 0), (10, 0, 0)], 8) == [0, 1, 1, 2]
    # a full group closes; max_group <= 1: one group per stamp
    row = [(i * R, 0, 0) for i in range(5)]
    assert c_plan(lib, 96, 1000, R, False, row, 2) == [0, 0, 1, 1, 2]
    assert c_plan(lib, 96, 1000, R, False, row, 8) == [0, 0, 0, 0, 0]
    for mg in (1, 0, -3):
        assert c_plan(lib, 96, 1000, R, False, row, mg) == [0, 1, 2, 3, 4]
    # an Erase stamp neither joins nor is joined
    assert c_plan(lib, 96, 1000, R, False, [(0, 0, 0), (R, 0, ERASE), (2 * R, 0, 0), (3 * R, 0, OVERPAINT)], 8) == [0, 1, 2, 2]
    assert c_plan(lib, 96, 1000, R, False, [(0, 0, ERASE), (R, 0, ERASE)], 8) == [0, 1]
    # the grouped stroke of tests/test_gpu_stroke.py
    assert c_plan(lib, H, W, R, False, [(0, 0, 0), (64, 0, 0), (32, 0, 0), (96, 16, 0)], 2) == [0, 0, 1, 1]


def test_python_wrapper(lib):
    from diffusiontexturepainting_amd.inpainter import plan_stroke
    pos = [(0, 0), (64, 0), (32, 0), (96, 16)]
    assert plan_stroke(pos, 96, 160, R, max_group=2) == [0, 0, 1, 1]
    assert plan_stroke(pos, 96, 160, R) == [0, 1, 2, 3]
    assert plan_stroke(pos, 96, 160, R, modes=["inpaint", "Erase", "overpaint", 0], max_group=2) == [0, 1, 2, 2]
    assert plan_stroke(pos, 96, 160, R, modes="erase", max_group=2) == [0, 1, 2, 3]
    assert plan_stroke([(128, 0), (31, 0)], 96, 160, R, wrap=True, max_group=2) == [0, 1]
    with pytest.raises(ValueError, match="brush mode"):
        plan_stroke(pos, 96, 160, R, modes="smudge")
    with pytest.raises(ValueError, match="modes"):
        plan_stroke(pos, 96, 160, R, modes=[0, 0])
    with pytest.raises(ValueError, match="at least one"):
        plan_stroke([], 96, 160, R)


def test_header_and_binding_agree_on_the_stroke_entry_points(lib):
    from diffusiontexturepainting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dtp.h")).read()
    assert re.search(r"#define\s+DTP_ABI_VERSION\s+3\b", hdr)
    assert lib.dtp_abi_version() == 3
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dtp_[a-z0-9_]+)\s*\(", code))
    new = {"dtp_stroke", "dtp_stroke_plan", "dtp_last_stroke_info", "dtp_op_stroke_gather", "dtp_op_stroke_paste"}
    assert new <= declared and declared == set(_lib.SYMBOLS)
    for name in new:
        assert hasattr(lib, name), f"libdtp.so does not export {name}"
    assert re.search(r"enum\s*\{\s*DTP_STROKE_INPAINT = 0, DTP_STROKE_ERASE = 1, DTP_STROKE_OVERPAINT = 2\s*\}", code)
    assert _lib.STROKE_MODES == dict(inpaint=INPAINT, erase=ERASE, overpaint=OVERPAINT)
    # the two structs as the header lays them out
    assert [f[0] for f in _lib.StrokeStamp._fields_] == ["x", "y", "mode", "slot", "seed"] and C.sizeof(_lib.StrokeStamp) == 24
    assert [f[0] for f in _lib.StrokeOpts._fields_] == ["wrap", "margin", "over_y", "over_x", "max_group", "sample_vae", "strength"]
    assert C.sizeof(_lib.StrokeOpts) == 32
    m = re.search(r"typedef struct \{([^}]*)\} dtp_stroke_stamp;", code)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "int x, y, mode, slot; uint64_t seed;"
    m = re.search(r"typedef struct \{([^}]*)\} dtp_stroke_opts;", code)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "int wrap, margin, over_y, over_x, max_group, sample_vae; double strength;"


def test_planner_argument_errors(lib):
    from diffusiontexturepainting_amd import _lib
    one = (_lib.StrokeStamp * 2)(_lib.StrokeStamp(0, 0, 0, 0, 0), _lib.StrokeStamp(5, 5, 0, 0, 0))
    out, ng = (C.c_int * 2)(9, 9), C.c_int(9)
    ARG = 1  # DTP_ERR_ARG

    def refused(rc, word):
        assert rc == ARG and word in lib.dtp_last_error().decode(), (rc, lib.dtp_last_error())
        assert list(out) == [9, 9] and ng.value == 9  # a refused call writes nothing

    refused(lib.dtp_stroke_plan(96, 160, R, 0, None, 2, 2, out, C.byref(ng)), "stamps")
    refused(lib.dtp_stroke_plan(96, 160, R, 0, one, 2, 2, None, C.byref(ng)), "group_of")
    refused(lib.dtp_stroke_plan(96, 160, R, 0, one, 0, 2, out, C.byref(ng)), "n=0")
    refused(lib.dtp_stroke_plan(96, 160, R, 0, one, -1, 2, out, C.byref(ng)), "n=-1")
    refused(lib.dtp_stroke_plan(63, 160, R, 0, one, 2, 2, out, C.byref(ng)), "smaller")
    refused(lib.dtp_stroke_plan(96, 63, R, 1, one, 2, 2, out, C.byref(ng)), "smaller")
    refused(lib.dtp_stroke_plan(96, 160, 0, 0, one, 2, 2, out, C.byref(ng)), "smaller")
    bad = (_lib.StrokeStamp * 2)(_lib.StrokeStamp(0, 0, 0, 0, 0), _lib.StrokeStamp(5, 5, 3, 0, 0))
    refused(lib.dtp_stroke_plan(96, 160, R, 0, bad, 2, 2, out, C.byref(ng)), "stamp 1")
    bad[1].mode = -1
    refused(lib.dtp_stroke_plan(96, 160, R, 0, bad, 2, 2, out, C.byref(ng)), "stamp 1")
    # n_groups is optional; H == W == R is the smallest texture
    assert lib.dtp_stroke_plan(R, R, R, 1, one, 2, 2, out, None) == 0 and list(out) == [0, 1]
