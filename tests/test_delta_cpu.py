"""The changed tiles of an image without a GPU (include/dtp.h: "changed tiles of an image"): dtp_delta_layout against the numpy restatement
(tests/delta_ref.py), the wire frame's codec -- round trips, every refusal of apply_frame with the mirror unchanged, and a hand-written
frame byte for byte --, the header's declarations against the ctypes binding, the refusals that need no device -- each must answer with
its message before the first device call, since there is no device here --, and the stand-alone host program tools/delta_host_check.cpp."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import delta_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dtp_delta_layout", "dtp_delta_create", "dtp_delta_destroy", "dtp_delta_reset", "dtp_delta_scan", "dtp_delta_device",
         "dtp_delta_host", "dtp_delta_pull", "dtp_op_delta_state"]
SIZES = [(1, 1), (16, 16), (17, 33), (90, 150), (96, 160), (16384, 16384)]


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


# ---------------------------------------------------------------- the header, the binding, the symbols
def test_symbols_are_declared_bound_and_exported(lib):
    from diffusiontexturepainting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dtp.h")).read()
    assert "changed tiles of an image" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        m = re.search(rf"\bint {name}\s*\(([^;]*)\);", hdr)
        assert m, name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == len(m.group(1).split(",")), name  # as many arguments as the header declares
    assert lib.dtp_abi_version() == 3  # entry points were added, nothing changed
    # the struct: the same fields in the same order, ints then 64-bit sizes
    m = re.search(r"typedef struct \{([^}]*)\} dtp_delta_sizes;", hdr)
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), {"int": C.c_int, "uint64_t": C.c_uint64}[ctype]) for n in names.split(",")]
    assert fields == list(_lib.DeltaSizes._fields_)


def test_the_module_imports_without_torch():
    """A client has neither torch nor a GPU: delta.py, as a client imports it, pulls in numpy and the standard library alone."""
    code = ("import sys; sys.modules['torch'] = None\n"
            "from diffusiontexturepainting_amd import delta\n"
            "import numpy as np\n"
            "m = np.zeros((20, 20, 4), np.uint8)\n"
            "b = delta.encode_frame(20, 20, 0, [3], np.full((1, 16, 16, 4), 9, np.uint8), first=True)\n"
            "assert delta.apply_frame(m, b) == (0, 0) and m[16:, 16:].min() == 9 and m[:16].max() == 0\n"
            "assert delta.decode_frame(b)['first']\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------- the layout
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_layout_equals_the_restatement(lib, size):
    from diffusiontexturepainting_amd import journal, ops
    H, W = size
    got = ops.delta_layout(H, W)
    assert got == delta_ref.layout(H, W)
    assert got["n_tiles"] == journal.tile_count(H, W) == got["tiles_x"] * got["tiles_y"] == got["capacity"]  # the journal's tiling
    assert ops.delta_layout(H, W, 7) == delta_ref.layout(H, W, 7)
    assert ops.delta_layout(H, W, 1)["host_bytes"] == 32 + 1024


def test_layout_refusals(lib):
    from diffusiontexturepainting_amd import _lib
    lay = _lib.DeltaSizes()
    C.memset(C.byref(lay), 0x77, C.sizeof(lay))
    before = bytes(lay)

    def refused(pattern, *args):
        assert lib.dtp_delta_layout(*args) == 1
        assert re.search(pattern, lib.dtp_last_error().decode()), lib.dtp_last_error()
        assert bytes(lay) == before

    refused("out is NULL", 90, 150, 5, None)
    refused("a 0 x 150 image", 0, 150, 5, C.byref(lay))
    refused("a 90 x -1 image", 90, -1, 5, C.byref(lay))
    refused(r"a 16385 x 150 image \(each side 1..16384\)", 16385, 150, 5, C.byref(lay))
    refused("a 90 x 16385 image", 90, 16385, 5, C.byref(lay))
    refused("capacity_tiles=0", 90, 150, 0, C.byref(lay))
    refused("capacity_tiles=-2", 90, 150, -2, C.byref(lay))


# ---------------------------------------------------------------- refusals that need no device
def test_create_refuses_before_any_device_call(lib):
    out = C.c_void_p()

    def refused(pattern, ctx, H, W, cap, outp=out):
        assert lib.dtp_delta_create(ctx, H, W, cap, C.byref(outp) if outp is not None else None) == 1
        assert re.search(pattern, lib.dtp_last_error().decode()), lib.dtp_last_error()
        assert not out.value

    refused("a 0 x 150 image", None, 0, 150, 8)
    refused("a 90 x 16385 image", None, 90, 16385, 8)
    refused("a -1 x 150 image", None, -1, 150, 8)
    refused("capacity_tiles=0", None, 90, 150, 0)
    refused("capacity_tiles=-5", None, 90, 150, -5)
    refused("out is NULL", None, 90, 150, 8, outp=None)
    refused("ctx is NULL", None, 90, 150, 8)  # every other argument is fine: only now is the handle looked at


def test_a_pointer_that_is_no_live_tracker_is_refused_and_not_followed(lib):
    junk = (C.c_uint8 * 4096)(*([0xAB] * 4096))  # followed, these bytes would be pointers into nowhere
    p = C.c_void_p(C.addressof(junk))
    ctx = C.c_void_p(C.addressof(junk) + 2048)  # never looked into either: the tracker is refused first
    img = (C.c_uint8 * 64)()
    ids, tiles = (C.c_int * 4)(*([-7] * 4)), (C.c_uint8 * 4096)(*([0xEE] * 4096))
    a, b, c = C.c_void_p(11), C.c_void_p(12), C.c_void_p(13)
    n, rem = C.c_int(-1), C.c_int(-1)
    calls = {
        "dtp_delta_reset": lambda q: lib.dtp_delta_reset(q, None),
        "dtp_delta_scan": lambda q: lib.dtp_delta_scan(ctx, q, img, 4, 4, None),
        "dtp_delta_device": lambda q: lib.dtp_delta_device(q, C.byref(a), C.byref(b), C.byref(c)),
        "dtp_delta_host": lambda q: lib.dtp_delta_host(q, C.byref(a), C.byref(b)),
        "dtp_delta_pull": lambda q: lib.dtp_delta_pull(ctx, q, img, 4, 4, None, ids, tiles, 4, C.byref(n), C.byref(rem)),
        "dtp_op_delta_state": lambda q: lib.dtp_op_delta_state(q, img, img, None),
    }
    for name, call in calls.items():
        assert call(p) == 1, name
        assert re.search(rf"{name}: not a live tracker", lib.dtp_last_error().decode()), lib.dtp_last_error()
        assert call(None) == 1, name
        assert re.search(rf"{name}: the tracker is NULL", lib.dtp_last_error().decode()), lib.dtp_last_error()
    assert (a.value, b.value, c.value, n.value, rem.value) == (11, 12, 13, -1, -1)
    assert list(ids) == [-7] * 4 and bytes(tiles) == b"\xee" * 4096
    # NULL outputs and a NULL handle are named before the tracker is looked at
    assert lib.dtp_delta_device(p, None, C.byref(b), C.byref(c)) == 1 and b"dtp_delta_device: NULL argument" in lib.dtp_last_error()
    assert lib.dtp_delta_host(p, C.byref(a), None) == 1 and b"dtp_delta_host: NULL argument" in lib.dtp_last_error()
    assert lib.dtp_delta_scan(None, p, img, 4, 4, None) == 1 and b"dtp_delta_scan: ctx is NULL" in lib.dtp_last_error()
    assert lib.dtp_delta_pull(None, p, img, 4, 4, None, ids, tiles, 4, C.byref(n), C.byref(rem)) == 1 and b"dtp_delta_pull: ctx is NULL" in lib.dtp_last_error()
    assert lib.dtp_delta_destroy(p) == 1 and b"not a live tracker" in lib.dtp_last_error()
    assert lib.dtp_delta_destroy(None) == 0  # a no-op
    assert bytes(junk) == b"\xab" * 4096


# ---------------------------------------------------------------- the wire frame
def random_frame(rng, H, W, k):
    n = delta_ref.layout(H, W)["n_tiles"]
    ids = np.sort(rng.choice(n, size=min(k, n), replace=False)).astype(np.int32)
    tiles = rng.integers(0, 256, (len(ids), 16, 16, 4), dtype=np.uint8)
    return ids, tiles


@pytest.mark.parametrize("size", [(1, 1), (16, 16), (17, 33), (90, 150), (96, 160)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_round_trip_onto_random_mirrors(size):
    from diffusiontexturepainting_amd import delta
    H, W = size
    rng = np.random.default_rng(H * 1000 + W)
    n = delta_ref.layout(H, W)["n_tiles"]
    mirror = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    want = mirror.copy()
    expect = None
    for seq, k in enumerate([0, 1, n // 2, n]):  # none, one, half, all: the edge tiles are among them
        ids, tiles = random_frame(rng, H, W, k)
        if k == 1:
            ids[:] = n - 1  # the corner tile, partial where the size is no multiple of 16
        b = delta.encode_frame(H, W, seq, ids, tiles, remaining=3 * k, first=seq == 0)
        assert b == delta_ref.encode(H, W, seq, ids, tiles, remaining=3 * k, first=seq == 0)  # the restatement writes the same bytes
        f = delta.decode_frame(b)
        assert (f["H"], f["W"], f["seq"], f["first"], f["remaining"]) == (H, W, seq, seq == 0, 3 * k)
        assert np.array_equal(f["ids"], ids) and np.array_equal(f["tiles"], tiles) and f["tiles"].shape == (len(ids), 16, 16, 4)
        assert delta.apply_frame(mirror, b, expect_seq=expect) == (seq, 3 * k)
        assert delta_ref.apply(want, b) == (seq, 3 * k)
        assert np.array_equal(mirror, want)
        for t, p in zip(ids.tolist(), tiles):  # written as far as the image goes, clipped at its edge
            r0, c0, rows, cols = delta_ref.tile_box(H, W, t)
            assert np.array_equal(mirror[r0:r0 + rows, c0:c0 + cols], p[:rows, :cols])
        expect = seq + 1
    assert delta.apply_frame(mirror, delta.encode_frame(H, W, 0xFFFFFFFF, [], np.zeros((0, 16, 16, 4), np.uint8)))[0] == 0xFFFFFFFF


def test_a_hand_written_frame_byte_for_byte():
    """Two tiles of a 17 x 33 image (3 x 2 tiles), written out by hand: the format cannot drift."""
    from diffusiontexturepainting_amd import delta
    t1 = np.arange(1024, dtype=np.uint32).astype(np.uint8).reshape(16, 16, 4)
    t5 = (255 - t1)
    by_hand = (b"DTPD" + b"\x01" + b"\x01" + b"\x10\x00"          # magic, version 1, flags: first, tile 16
               + b"\x21\x00\x00\x00" + b"\x11\x00\x00\x00"        # W = 33, H = 17
               + b"\x2a\x00\x00\x00"                              # seq 42
               + b"\x02\x00\x00\x00" + b"\x07\x00\x00\x00"        # count 2, remaining 7
               + b"\x01\x00\x00\x00" + b"\x05\x00\x00\x00"        # ids 1, 5
               + bytes(range(256)) * 4 + bytes(range(255, -1, -1)) * 4)
    assert len(by_hand) == 28 + 2 * 1028
    assert delta.encode_frame(17, 33, 42, [1, 5], np.stack([t1, t5]), remaining=7, first=True) == by_hand
    f = delta.decode_frame(by_hand)
    assert (f["H"], f["W"], f["seq"], f["first"], f["remaining"], f["ids"].tolist()) == (17, 33, 42, True, 7, [1, 5])
    assert f["ids"].dtype == np.int32 and f["tiles"].dtype == np.uint8
    mirror = np.zeros((17, 33, 4), np.uint8)
    assert delta.apply_frame(mirror, by_hand, expect_seq=42) == (42, 7)
    want = np.zeros((17, 33, 4), np.uint8)
    want[0:16, 16:32] = t1           # tile 1: row 0 of tiles, columns 16 .. 31
    want[16:17, 32:33] = t5[:1, :1]  # tile 5: the corner, one texel of it inside
    assert np.array_equal(mirror, want)
    assert delta.HEADER.size == 28 and struct.calcsize("<4sBBHiiIii") == 28


def test_apply_frame_refuses_and_leaves_the_mirror_alone():
    from diffusiontexturepainting_amd import delta
    rng = np.random.default_rng(3)
    H, W = 17, 33
    mirror = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    before = mirror.copy()
    tiles = rng.integers(0, 256, (2, 16, 16, 4), dtype=np.uint8)
    good = delta_ref.encode(H, W, 5, [1, 5], tiles)
    bad = {
        "magic": (delta_ref.encode(H, W, 5, [1, 5], tiles, magic=b"DTPX"), "magic"),
        "version": (delta_ref.encode(H, W, 5, [1, 5], tiles, version=2), "version"),
        "tile_size": (delta_ref.encode(H, W, 5, [1, 5], tiles, tile=32), "tile size"),
        "another_shape": (delta_ref.encode(H, W + 1, 5, [1, 5], tiles), "the mirror is 17 x 33"),
        "transposed_shape": (delta_ref.encode(W, H, 5, [1, 5], tiles), "the mirror is 17 x 33"),
        "count_too_large": (delta_ref.encode(H, W, 5, [1, 5], tiles, count=3), "bytes"),
        "count_too_small": (delta_ref.encode(H, W, 5, [1, 5], tiles, count=1), "bytes"),
        "negative_count": (delta_ref.encode(H, W, 5, [], tiles[:0], count=-1), "negative"),
        "truncated": (good[:-1], "bytes"),
        "one_byte_more": (good + b"\0", "bytes"),
        "header_cut": (good[:20], "at least 28"),
        "id_outside": (delta_ref.encode(H, W, 5, [1, 6], tiles), "outside 0..5"),
        "negative_id": (delta_ref.encode(H, W, 5, [-1, 5], tiles), "outside 0..5"),
        "descending_ids": (delta_ref.encode(H, W, 5, [5, 1], tiles), "ascend"),
        "repeated_id": (delta_ref.encode(H, W, 5, [1, 1], tiles), "ascend"),
    }
    for name, (b, pattern) in bad.items():
        with pytest.raises(ValueError, match=pattern):
            delta.apply_frame(mirror, b)
        assert np.array_equal(mirror, before), name
    with pytest.raises(ValueError, match="sequence gap: frame 5, expected 6"):
        delta.apply_frame(mirror, good, expect_seq=6)
    with pytest.raises(ValueError, match="sequence gap"):
        delta.apply_frame(mirror, good, expect_seq=4)
    assert np.array_equal(mirror, before)
    with pytest.raises(ValueError, match="mirror must be"):
        delta.apply_frame(mirror.astype(np.int32), good)
    assert delta.apply_frame(mirror, good, expect_seq=5) == (5, 0) and not np.array_equal(mirror, before)


# ---------------------------------------------------------------- the restatement itself
def test_restatement_scan_caps_continues_and_forgets_a_change_made_back():
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (90, 150, 4), dtype=np.uint8)
    t = delta_ref.Tracker(90, 150, capacity=25)
    mirror = np.zeros_like(img)
    got = []
    for want_counts in ([25, 35], [25, 10], [10, 0], [0, 0]):
        ids, tiles, counts = t.scan(img)
        assert counts == want_counts
        got += ids.tolist()
        delta_ref.apply(mirror, delta_ref.encode(90, 150, 0, ids, tiles))
    assert got == list(range(60)) and np.array_equal(mirror, img) and not t.stale.any() and np.array_equal(t.shadow, img)
    img[89, 149, 3] ^= 1
    ids, tiles, counts = t.scan(img)
    assert ids.tolist() == [59] and counts == [1, 0] and not tiles[0, 10:].any() and not tiles[0, :, 6:].any()  # zero outside the image
    img[5, 5, 0] ^= 1
    img[5, 5, 0] ^= 1
    assert t.scan(img)[2] == [0, 0]
    t.reset()
    assert t.scan(img)[2] == [25, 35]


# ---------------------------------------------------------------- the stand-alone host program
def test_host_check_program_builds_and_passes(tmp_path):
    """tools/delta_host_check.cpp drives csrc/delta_host.h from its own main().  Here it is built plainly and run; the sanitizer run is
    the same program, built and run by hand (never from pytest, never with a preload):
        c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I diffusiontexturepainting_amd/csrc \\
            tools/delta_host_check.cpp -o delta_host_check && ./delta_host_check
    """
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "delta_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "diffusiontexturepainting_amd", "csrc"),
                        os.path.join(ROOT, "tools", "delta_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "checks passed" in r.stdout, r.stdout + r.stderr
