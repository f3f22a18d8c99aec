"""The host-only part of the bleed pass of the mesh strokes (include/dtp.h: dtp_mesh_bleed_offsets and the header against the binding)
and the restatement the GPU tests compare with (tests/bleed_ref.py): its own properties on the two-chart height field, and the figure
the pass exists for -- the alpha a second render sees along a UV seam, without and with the gutter filled.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import bleed_ref
import mesh_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1  # DTP_ERR_ARG
H, W = 96, 160


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def field():
    from diffusiontexturepainting_amd import synthetic
    return synthetic.make_height_field(17, 13, seed=3)


@pytest.fixture(scope="module")
def cov(field):
    return bleed_ref.coverage(field[2], H, W)


@pytest.fixture(scope="module")
def texture():
    return torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(21))


# ---------------------------------------------------------------- the offset table
def test_offsets_equal_the_restatement_for_every_radius(lib):
    from diffusiontexturepainting_amd import ops
    previous = None
    for k in range(1, 17):
        got = ops.mesh_bleed_offsets(k).numpy()
        want = bleed_ref.offsets(k)
        assert got.dtype == np.int8 and got.shape == want.shape and (got == want).all(), k
        d2 = (got.astype(np.int64) ** 2).sum(axis=1)
        assert d2.min() >= 1 and d2.max() <= k * k
        # the count: the lattice points of the disc without its centre
        assert len(got) == sum(1 for a in range(-k, k + 1) for b in range(-k, k + 1) if 0 < a * a + b * b <= k * k)
        # the contract's key rises strictly
        key = [(int(d), int(a), int(b)) for d, (a, b) in zip(d2, got)]
        assert key == sorted(key) and len(set(key)) == len(key)
        if previous is not None:
            assert (got[:len(previous)] == previous).all()  # each table is a prefix of the next
        previous = got
    assert len(previous) == 796
    assert ops.mesh_bleed_offsets(1).tolist() == [[-1, 0], [0, -1], [0, 1], [1, 0]]
    assert ops.mesh_bleed_offsets(2).tolist() == [[-1, 0], [0, -1], [0, 1], [1, 0], [-1, -1], [-1, 1], [1, -1], [1, 1],
                                                   [-2, 0], [0, -2], [0, 2], [2, 0]]
    n = C.c_int(-1)
    assert lib.dtp_mesh_bleed_offsets(3, C.byref(n), None) == 0 and n.value == 28  # the count alone


def test_offsets_refusals(lib):
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd._lib import DtpError
    n = C.c_int(-7)
    buf = (C.c_byte * 1600)(*([9] * 1600))
    for radius in (0, 17, -1):
        assert lib.dtp_mesh_bleed_offsets(radius, C.byref(n), buf) == ARG and b"radius" in lib.dtp_last_error()
        with pytest.raises(DtpError, match=rf"\(code {ARG}\).*radius"):
            ops.mesh_bleed_offsets(radius)
        with pytest.raises(ValueError):
            bleed_ref.offsets(radius)
    assert lib.dtp_mesh_bleed_offsets(4, None, buf) == ARG and b"NULL" in lib.dtp_last_error()
    assert n.value == -7 and set(buf) == {9}  # a refused call writes nothing


def test_header_and_binding_agree_on_the_bleed_entry_points(lib):
    from diffusiontexturepainting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dtp.h")).read()
    assert re.search(r"#define\s+DTP_ABI_VERSION\s+3\b", hdr)
    assert lib.dtp_abi_version() == 3
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dtp_[a-z0-9_]+)\s*\(", code))
    new = {"dtp_mesh_stroke_bleed", "dtp_mesh_bleed", "dtp_op_mesh_coverage", "dtp_mesh_bleed_offsets"}
    assert new <= declared and declared == set(_lib.SYMBOLS)
    for name in new:
        assert hasattr(lib, name), f"libdtp.so does not export {name}"
    # dtp_mesh_stroke_bleed is dtp_mesh_stroke with `int bleed` before the stream, in the header and in the binding
    flat = re.sub(r"\s+", " ", code)
    plain = re.search(r"int dtp_mesh_stroke\(([^)]*)\)", flat).group(1)
    bled = re.search(r"int dtp_mesh_stroke_bleed\(([^)]*)\)", flat).group(1)
    assert bled == plain.replace(", dtp_stream s", ", int bleed, dtp_stream s")
    a, b = _lib.SYMBOLS["dtp_mesh_stroke"], _lib.SYMBOLS["dtp_mesh_stroke_bleed"]
    assert b[0] is a[0] and b[1] == a[1][:-1] + [C.c_int, a[1][-1]]
    # the existing structures stay byte for byte
    assert C.sizeof(_lib.MeshStamp) == 56 and C.sizeof(_lib.MeshStrokeOpts) == 32
    assert re.search(r"int dtp_mesh_bleed\(dtp_mesh\* mesh, uint8_t\* texture, int H, int W, int bleed, const int\* rect, dtp_stream s\)", flat)
    assert re.search(r"int dtp_op_mesh_coverage\(dtp_mesh\* mesh, int H, int W, uint8_t\* out, dtp_stream s\)", flat)
    assert re.search(r"int dtp_mesh_bleed_offsets\(int radius, int\* count, signed char\* di_dj\)", flat)


def test_entry_points_refuse_bad_arguments_before_any_device_call(lib):
    """The argument checks that precede the look at the mesh run without a device: a handle that is not a live mesh is refused last."""
    tex = (C.c_uint32 * 4)()
    fake = (C.c_int * 64)()
    vp = (lambda a: C.cast(a, C.c_void_p))

    def refused(rc, word):
        assert rc == ARG and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())

    refused(lib.dtp_mesh_bleed(None, vp(tex), 2, 2, 1, None, None), "NULL")
    refused(lib.dtp_mesh_bleed(vp(fake), None, 2, 2, 1, None, None), "NULL")
    refused(lib.dtp_mesh_bleed(vp(fake), vp(tex), 2, 2, 17, None, None), "bleed=17")
    refused(lib.dtp_mesh_bleed(vp(fake), vp(tex), 2, 2, -1, None, None), "bleed=-1")
    refused(lib.dtp_mesh_bleed(vp(fake), vp(tex), 0, 2, 1, None, None), "0 x 2 texture")
    refused(lib.dtp_mesh_bleed(vp(fake), vp(tex), 2, 2, 1, C.byref((C.c_int * 4)(1, 0, 0, 1)), None), "x0 > x1")
    refused(lib.dtp_mesh_bleed(vp(fake), vp(tex), 2, 2, 1, C.byref((C.c_int * 4)(0, 1, 1, 0)), None), "y0 > y1")
    refused(lib.dtp_mesh_bleed(vp(fake), vp(tex), 2, 2, 1, None, None), "not a live mesh")
    refused(lib.dtp_op_mesh_coverage(None, 2, 2, vp(tex), None), "NULL")
    refused(lib.dtp_op_mesh_coverage(vp(fake), 2, 2, None, None), "NULL")
    refused(lib.dtp_op_mesh_coverage(vp(fake), 2, 40000, vp(tex), None), "2 x 40000")
    refused(lib.dtp_op_mesh_coverage(vp(fake), 2, 2, vp(tex), None), "not a live mesh")
    # the radius of a stroke is looked at before anything else is
    refused(lib.dtp_mesh_stroke_bleed(None, None, None, 2, 2, None, 1, None, None, None, 17, None), "dtp_mesh_stroke_bleed: bleed=17")
    refused(lib.dtp_mesh_stroke_bleed(None, None, None, 2, 2, None, 1, None, None, None, -1, None), "bleed=-1")
    refused(lib.dtp_mesh_stroke_bleed(None, None, None, 2, 2, None, 1, None, None, None, 2, None), "NULL")


# ---------------------------------------------------------------- the restatement's own properties
def test_batched_coverage_equals_the_rasterised_one(field):
    from diffusiontexturepainting_amd import synthetic
    for uv, sizes in ((field[2], ((H, W), (75, 101), (1, 1), (7, 300))), (synthetic.make_quad()[2], ((64, 64), (1, 1), (33, 47)))):
        for h, w in sizes:
            assert (bleed_ref.coverage_batched(uv, h, w) == bleed_ref.coverage(uv, h, w)).all(), (h, w)
            assert (bleed_ref.coverage_batched(uv, h, w, budget=64) == bleed_ref.coverage(uv, h, w)).all(), (h, w)
    assert bleed_ref.coverage(synthetic.make_quad()[2], 33, 47).all()  # the shared diagonal leaves no hole


def test_coverage_of_the_two_chart_field_has_a_middle_gutter(cov):
    # u in [0.03, 0.47] and [0.53, 0.97], v in [0.05, 0.95]: two solid charts, a gutter between them and a border around them
    cols = np.nonzero(cov.any(axis=0))[0]
    rows = np.nonzero(cov.any(axis=1))[0]
    assert cols.min() == 5 and cols.max() == 154 and rows.min() == 5 and rows.max() == 90
    gutter = np.nonzero(~cov[40])[0]
    middle = gutter[(gutter > 60) & (gutter < 100)]
    assert middle.tolist() == list(range(75, 85))
    assert cov[5:91, 5:75].all() and cov[5:91, 85:155].all()  # no hole on any shared edge


@pytest.mark.parametrize("k", [1, 2, 5, 16])
def test_the_pass_is_idempotent_reads_covered_and_writes_uncovered(cov, texture, k):
    once = bleed_ref.bleed(texture, cov, k)
    assert torch.equal(bleed_ref.bleed(once, cov, k), once)
    changed = (once != texture).any(dim=-1).numpy()
    assert changed.any() and not (changed & cov).any()
    has, si, sj = bleed_ref.source(cov, k)
    assert not (has & cov).any() and cov[si[has], sj[has]].all()
    assert torch.equal(once[torch.from_numpy(has)], texture[torch.from_numpy(si[has]), torch.from_numpy(sj[has])])
    # a source is a nearest covered texel within the radius, and every gutter texel that has one within the radius has a source
    ii, jj = np.nonzero(cov)
    for i, j in [(40, 75), (40, 79), (40, 84), (2, 2), (4, 100), (93, 154), (0, 0), (95, 159)]:
        d2 = (ii - i) ** 2 + (jj - j) ** 2
        if d2.min() <= k * k:
            assert has[i, j] and (si[i, j] - i) ** 2 + (sj[i, j] - j) ** 2 == d2.min()
        else:
            assert not has[i, j] and torch.equal(once[i, j], texture[i, j])


def test_a_tie_in_the_middle_gutter_goes_to_the_smaller_offset(cov, texture):
    # columns 75 .. 84 are the gutter: texel (40, 79) is 5 from column 74 and 6 from 85; (40, 80) the other way round; with an even
    # gutter there is no horizontal tie, so cut one column off the right chart
    c = cov.copy()
    c[:, 85] = False  # the gutter is now 75 .. 85, 11 wide: (40, 80) is 6 from both charts
    has, si, sj = bleed_ref.source(c, 6)
    assert has[40, 80] and (si[40, 80], sj[40, 80]) == (40, 74)  # (0, -6) before (0, 6)
    out = bleed_ref.bleed(texture, c, 6)
    assert torch.equal(out[40, 80], texture[40, 74]) and not torch.equal(texture[40, 74], texture[40, 86])
    # a corner of the border: (4, 4) is at distance^2 2 from (5, 5) only; (4, 5) takes (5, 5) at (1, 0)
    has, si, sj = bleed_ref.source(cov, 2)
    assert (si[4, 4], sj[4, 4]) == (5, 5) and (si[4, 5], sj[4, 5]) == (5, 5)
    # below the charts (row 91) at radius 2: (-1, 0) wins over (-1, -1) and (-1, 1)
    assert (si[91, 40], sj[91, 40]) == (90, 40)
    # a vertical tie: an uncovered row between two covered ones takes the upper (di = -1 before di = 1)
    c = cov.copy()
    c[50, :] = False
    has, si, sj = bleed_ref.source(c, 1)
    assert (si[50, 30], sj[50, 30]) == (49, 30)


def test_a_rectangle_bounds_what_is_written(cov, texture):
    rect = (70, 30, 90, 47)
    out = bleed_ref.bleed(texture, cov, 5, rect)
    changed = (out != texture).any(dim=-1).numpy()
    inside = np.zeros((H, W), dtype=bool)
    inside[30:48, 70:91] = True
    assert changed.any() and not (changed & ~inside).any()
    whole = bleed_ref.bleed(texture, cov, 5)
    assert torch.equal(out[30:48, 70:91], whole[30:48, 70:91])  # sources may lie outside the rectangle


# ---------------------------------------------------------------- what the pass is for
def test_the_seam_a_second_render_sees_closes_with_the_gutter_filled():
    """A blank 256^2 texture, one backprojection of a constant image over the default height field, and a second render of the same
    window: along the seam between the two charts the canvas alpha -- the inpainting mask of the next stamp -- drops to 0.9718 where a
    bilinear tap reaches into the gutter (125 of the 2304 interior pixels are below 0.999).  With the gutter filled from the nearest
    covered texel at radius 1, 2 or 4 the minimum is 0.99715, and the 29 pixels left below 0.999 sample painted texels whose alpha byte
    is 254, the backprojection's own truncation: not gutter."""
    from diffusiontexturepainting_amd import synthetic
    R, T = 64, 256
    v, f, uv = synthetic.make_height_field()
    cam = mesh_ref.camera((0, 0, 0.2), (0, 0, 1), (0, -1, 0.2), 0.45)  # looking down -z
    blank = torch.zeros(T, T, 4, dtype=torch.uint8)
    _, face_idx, proj = mesh_ref.render(v, f, uv, cam, 0.45, blank, R)
    painted = torch.full((3, R, R), 0.5)
    mask = torch.ones(R, R, dtype=torch.uint8)
    pasted, info = mesh_ref.backproject(proj, face_idx, uv, None, mask, blank, painted=painted)
    cover = bleed_ref.coverage(uv, T, T)
    assert not (info["written"] & ~cover).any()
    interior = np.zeros((R, R), dtype=bool)
    interior[8:R - 8, 8:R - 8] = True
    interior &= face_idx.numpy() != -1
    assert int(interior.sum()) == 2304

    def seam(tex):
        canvas, _, _ = mesh_ref.render(v, f, uv, cam, 0.45, tex, R)
        alpha = canvas[0, 3].numpy()[interior]
        return float(alpha.min()), int((alpha < 0.999).sum())

    low, n_low = seam(pasted)
    print(f"no bleed: min interior alpha {low:.5f}, {n_low} of 2304 below 0.999")
    assert low < 0.98 and n_low > 29
    for k in (1, 2, 4):
        rect = bleed_ref.stamp_rect(proj, face_idx, uv, T, T, k)
        filled = bleed_ref.bleed(pasted, cover, k, rect)
        got, n_got = seam(filled)
        print(f"bleed {k}: min interior alpha {got:.5f}, {n_got} of 2304 below 0.999")
        assert got >= 254 / 255 - 1e-6 and n_got < n_low
