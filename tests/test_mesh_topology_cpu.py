"""The host-only part of growing a face set (include/dtp.h "growing a face set") and the reference the GPU tests use
(tests/topo_ref.py): dtp_topology_build against the numpy restatement on meshes whose answer is known, a face permutation, the
properties of the reference's extends, every refusal that needs no device, the header against the binding, and the stand-alone host
program tools/topo_host_check.cpp.  Every comparison is ==.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import topo_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1  # DTP_ERR_ARG


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def meshes():
    """name -> (vertices, faces, face_uvs) as numpy: the meshes of the issue's list."""
    from diffusiontexturepainting_amd import synthetic
    out = {"quad": synthetic.make_quad(), "table_on_floor": synthetic.make_table_on_floor(), "field_50": synthetic.make_height_field(6, 6),
           "field_384": synthetic.make_height_field(17, 13, seed=3)}
    out = {k: tuple(t.numpy() for t in m) for k, m in out.items()}
    out["field_50_split_seam"] = topo_ref.split_seam(*out["field_50"])
    out["fan"] = topo_ref.fan()
    out["touching"] = topo_ref.touching()
    out["touching_degenerate"] = topo_ref.touching(degenerate=True)
    return out


MESHES = meshes()
# name -> (faces, distinct points, parts, the sizes of the charts in the order of their labels)
KNOWN = {"quad": (2, 4, 1, [2]), "table_on_floor": (4, 8, 2, [2, 2]), "field_50": (50, 36, 1, [20, 30]), "field_384": (384, 221, 1, [192, 192]),
         "field_50_split_seam": (50, 36, 1, [20, 30]), "fan": (3, 5, 1, [2, 1]), "touching": (2, 5, 1, [1, 1]),
         "touching_degenerate": (4, 5, 1, [2, 1, 1])}


def build(mesh):
    from diffusiontexturepainting_amd import mesh as M
    return M.topology_build(*[torch.from_numpy(np.ascontiguousarray(a)) for a in mesh])


def same_topology(a, b):
    return all((a[k] == b[k]).all() if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in ("point", "part", "chart", "num_points",
                                                                                                  "num_parts", "num_charts", "num_faces"))


# ---------------------------------------------------------------- the topology
@pytest.mark.parametrize("name", sorted(MESHES))
def test_topology_build_equals_the_restatement_and_what_is_known(name):
    v, f, uv = MESHES[name]
    got, ref = build(MESHES[name]), topo_ref.topology(v, f, uv)
    assert got["point"].dtype == np.int32 and got["point"].shape == (f.shape[0], 3) and got["part"].shape == got["chart"].shape == (f.shape[0],)
    assert same_topology(got, ref)
    F, n_points, n_parts, chart_sizes = KNOWN[name]
    assert (got["num_faces"], got["num_points"], got["num_parts"], got["num_charts"]) == (F, n_points, n_parts, len(chart_sizes))
    # counts are the numbers of distinct labels, and a label is the lowest index of its class
    assert len(np.unique(got["point"])) == n_points and len(np.unique(got["part"])) == n_parts
    labels, sizes = np.unique(got["chart"], return_counts=True)
    assert sizes.tolist() == chart_sizes
    for key in ("part", "chart"):
        assert (got[key] <= np.arange(F)).all() and (got[key][got[key]] == got[key]).all()
    assert (got["point"] <= f).all() and (v[got["point"]] == v[f]).all()  # (float ==: -0.0 equals +0.0)
    assert (got["part"][got["chart"]] == got["part"]).all()  # a chart never spans two parts
    if name == "table_on_floor":
        assert got["part"].tolist() == [0, 0, 2, 2] and got["chart"].tolist() == [0, 0, 2, 2]
    if name == "field_50":  # the faces left of the middle column are the first chart
        assert (got["chart"] == np.where(np.arange(50) % 10 < 4, 0, 4)).all()
    if name == "field_50_split_seam":
        shared = build(MESHES["field_50"])
        assert (got["part"] == shared["part"]).all() and (got["chart"] == shared["chart"]).all()
        assert v.shape[0] == 42 and got["num_points"] == 36 < v.shape[0] and int(got["point"].max()) < 36
        assert np.signbit(v[36:, 0]).any() and not np.signbit(v[:36][v[:36, 0] == 0, 0]).any()  # -0.0 against +0.0
    if name == "fan":
        assert got["chart"].tolist() == [0, 1, 0]
    if name == "touching":
        assert got["chart"].tolist() == [0, 1]
    if name == "touching_degenerate":
        assert got["chart"].tolist() == [0, 1, 0, 3] and got["part"].tolist() == [0, 0, 0, 0]


def test_a_face_permutation_gives_the_same_partition():
    v, f, uv = MESHES["field_384"]
    base = build(MESHES["field_384"])
    perm = np.random.default_rng(11).permutation(384)  # new face i is old face perm[i]
    got = build((v, f[perm], uv[perm]))
    assert same_topology(got, topo_ref.topology(v, f[perm], uv[perm]))
    for key in ("part", "chart"):
        # two new faces share a label exactly when the old faces did
        assert ((got[key][:, None] == got[key][None, :]) == (base[key][perm][:, None] == base[key][perm][None, :])).all()
        # and each label is still the lowest index of its class
        for label in np.unique(got[key]):
            assert label == np.nonzero(got[key] == label)[0].min()
    assert got["num_parts"] == 1 and got["num_charts"] == 2 and got["num_points"] == base["num_points"]


# ---------------------------------------------------------------- the reference's extends
def sets(F, seed=5):
    g = np.random.default_rng(seed)
    out = {f"random_{d}": g.random(F) < d for d in (0.02, 0.1, 0.5)}
    out.update(empty=np.zeros(F, dtype=bool), full=np.ones(F, dtype=bool), one_face=np.arange(F) == F // 3, last_face=np.arange(F) == F - 1)
    return out


def rings_to_fixed_point(topo, sel):
    """(the fixed point of rings, the number of rings that reached it)"""
    n = 0
    while True:
        new = topo_ref.extend(topo, sel, "rings", 1)
        if (new == sel).all():
            return sel, n
        sel, n = new, n + 1


@pytest.mark.parametrize("name", ["table_on_floor", "field_50", "field_384", "touching_degenerate"])
def test_properties_of_the_reference(name):
    topo = topo_ref.topology(*MESHES[name])
    F = topo["num_faces"]
    for which, sel in sets(F).items():
        linked = topo_ref.extend(topo, sel, "linked")
        assert (linked == rings_to_fixed_point(topo, sel)[0]).all(), which
        for n in (1, 2, 5):
            assert (topo_ref.extend(topo, sel, "shrink", n) == ~topo_ref.extend(topo, ~sel, "rings", n)).all(), which
            assert (topo_ref.extend(topo, sel, "rings", n) >= sel).all() and (topo_ref.extend(topo, sel, "shrink", n) <= sel).all()
        charts = topo_ref.extend(topo, sel, "charts")
        assert (charts <= linked).all() and (sel <= charts).all(), which
        if which == "empty":
            assert not any(topo_ref.extend(topo, sel, how, 3).any() for how in ("rings", "shrink", "linked", "charts"))
        if which == "full":
            assert all(topo_ref.extend(topo, sel, how, 3).all() for how in ("rings", "shrink", "linked", "charts"))
    if name == "table_on_floor":
        assert np.nonzero(topo_ref.extend(topo, np.arange(4) == 2, "linked"))[0].tolist() == [2, 3]
        assert np.nonzero(topo_ref.extend(topo, np.arange(4) == 2, "rings", 64))[0].tolist() == [2, 3]


@pytest.mark.parametrize("name,nx,ny", [("field_50", 6, 6), ("field_384", 17, 13)])
def test_rings_from_a_corner_reach_the_whole_field_within_the_cap(name, nx, ny):
    topo = topo_ref.topology(*MESHES[name])
    F = topo["num_faces"]
    whole, n = rings_to_fixed_point(topo, np.arange(F) == 0)
    assert whole.all() and 1 < n <= max(nx, ny) - 1 <= 64
    assert (topo_ref.extend(topo, np.arange(F) == 0, "rings", max(nx, ny) - 1) == topo_ref.extend(topo, np.arange(F) == 0, "linked")).all()


# ---------------------------------------------------------------- refusals, before any device call
def refused(lib, rc, word):
    assert rc == ARG and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())


def test_extend_refuses_a_bad_how_or_rings_before_the_mesh_is_looked_at(lib):
    """how and rings are checked first, so the checks run without a device: with mesh = NULL, which a good call then meets."""
    for how in (4, -1, 17):
        refused(lib, lib.dtp_mesh_select_extend(None, None, None, 1, how, 1, None), rf"unknown how {how}")
    for how in (0, 1):
        for rings in (0, 65, -1):
            refused(lib, lib.dtp_mesh_select_extend(None, None, None, 1, how, rings, None), rf"rings={rings} \(1\.\.64\)")
    for how, rings in ((0, 1), (1, 64), (2, 0), (3, 1000)):  # good, and rings is ignored by LINKED and CHARTS: now the pointers
        refused(lib, lib.dtp_mesh_select_extend(None, None, None, 1, how, rings, None), r"NULL")
    refused(lib, lib.dtp_mesh_topology(None, None, None), r"NULL")
    refused(lib, lib.dtp_mesh_topology_labels(None, None, None, None, None), r"NULL")


def test_topology_build_refusals(lib):
    v, f, uv = (np.ascontiguousarray(a).copy() for a in MESHES["field_50"])
    F, V = f.shape[0], v.shape[0]
    point, part, chart, counts = np.zeros((F, 3), np.int32), np.zeros(F, np.int32), np.zeros(F, np.int32), (C.c_int * 3)()
    p = (lambda a: C.c_void_p(a.ctypes.data))

    def call(v_=v, V_=V, f_=f, F_=F, uv_=uv, out=(point, part, chart), counts_=counts):
        return lib.dtp_topology_build(None if v_ is None else p(v_), V_, None if f_ is None else p(f_), F_, None if uv_ is None else p(uv_),
                                      *[None if o is None else p(o) for o in out], None if counts_ is None else C.byref(counts_))

    assert call() == 0 and list(counts) == [36, 1, 2]
    for kw in (dict(v_=None), dict(f_=None), dict(uv_=None), dict(out=(None, part, chart)), dict(out=(point, None, chart)),
               dict(out=(point, part, None)), dict(counts_=None)):
        refused(lib, call(**kw), r"NULL")
    refused(lib, call(F_=0), r"F=0 faces")
    refused(lib, call(F_=-3), r"F=-3 faces")
    refused(lib, call(F_=(1 << 20) + 1), r"F=1048577 faces")  # (refused before a face is read)
    refused(lib, call(V_=0), r"V=0 vertices")
    for value, word in ((V, rf"face 7 refers to vertex {V} \(0\.\.{V - 1}\)"), (-1, r"face 7 refers to vertex -1")):
        bad = f.copy()
        bad[7, 2] = value
        refused(lib, call(f_=bad), word)
    for value in (float("nan"), float("inf"), float("-inf")):
        bad = v.copy()
        bad[5, 1] = value
        refused(lib, call(v_=bad), r"vertex 5 is not finite")
        bad = uv.copy()
        bad[9, 2, 0] = value
        refused(lib, call(uv_=bad), r"face 9 has a UV that is not finite")
    from diffusiontexturepainting_amd import mesh as M
    from diffusiontexturepainting_amd._lib import DtpError
    with pytest.raises(DtpError, match="F=0 faces"):
        M.topology_build(torch.zeros(3, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3, 2))
    with pytest.raises(ValueError, match=r"faces \[F, 3\]"):
        M.topology_build(torch.zeros(3, 3), torch.zeros(3, dtype=torch.int32), torch.zeros(1, 3, 2))


def test_extend_keywords_are_checked_before_any_device_call():
    from diffusiontexturepainting_amd import inpainter
    assert inpainter._extend_args("charts", 3) == ("charts", 3)
    with pytest.raises(ValueError, match="how 'grow'"):
        inpainter._extend_args("grow", 1)
    for rings in (1.0, True, None, "2"):
        with pytest.raises(ValueError, match="rings"):
            inpainter._extend_args("rings", rings)


# ---------------------------------------------------------------- header, binding, host program
def test_header_and_binding_agree_on_the_extend_entry_points(lib):
    from diffusiontexturepainting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dtp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dtp_[a-z0-9_]+)\s*\(", code))
    new = {"dtp_topology_build", "dtp_mesh_topology", "dtp_mesh_topology_labels", "dtp_mesh_select_extend"}
    assert new <= declared and declared == set(_lib.SYMBOLS)
    for name in new:
        assert hasattr(lib, name), f"libdtp.so does not export {name}"
        # the binding passes as many arguments as the header declares
        params = re.search(rf"\b{name}\s*\(([^)]*)\)", code).group(1)
        assert len(params.split(",")) == len(_lib.SYMBOLS[name][1]), name
    assert sorted(_lib.EXTEND_HOWS.values()) == [0, 1, 2, 3]
    for name, value in _lib.EXTEND_HOWS.items():
        assert re.search(rf"#define\s+DTP_EXTEND_{name.upper()}\s+{value}\b", hdr)
    assert lib.dtp_abi_version() == 3


def test_host_check_program_builds_and_passes(tmp_path):
    """tools/topo_host_check.cpp drives csrc/topo_host.h from its own main().  Here it is built plainly and run; the sanitizer run is the
    same program, built and run by hand (never from pytest, never with a preload):
        c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I diffusiontexturepainting_amd/csrc \\
            tools/topo_host_check.cpp -o topo_host_check && ./topo_host_check
    """
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "topo_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "diffusiontexturepainting_amd", "csrc"),
                        os.path.join(ROOT, "tools", "topo_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "checks passed" in r.stdout, r.stdout + r.stderr
