"""The undo / redo journal without a GPU (include/dtp.h: "undo / redo journal of a texture"): the host-only tile list of a 2D stroke window
against the numpy restatement (tests/journal_ref.py), the refusals that need no device -- each must answer with its message before the
first device call, since there is no device here --, the exported symbols, the restatement's own state machine, and the stand-alone host
program tools/journal_host_check.cpp."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import journal_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dtp_journal_create", "dtp_journal_destroy", "dtp_journal_begin", "dtp_journal_end", "dtp_journal_touch", "dtp_journal_undo",
         "dtp_journal_redo", "dtp_journal_info", "dtp_journal_record_info", "dtp_op_journal_tiles", "dtp_journal_window_tiles"]


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    from diffusiontexturepainting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dtp.h")).read()
    assert "undo / redo journal of a texture" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.dtp_abi_version() == 3  # entry points were added, nothing changed


# ---------------------------------------------------------------- window -> tiles
# (H, W, R, x, y, wrap): inside; partly outside on every side; on one tile; outside; wrapped across each border and the corner; W = R and
# W = R + 8, where the two wrapped pieces share a tile; 90 x 150 with its partial edge tiles
WINDOWS = [
    (96, 160, 64, 16, 16, False), (96, 160, 64, 20, 9, False), (96, 160, 64, 96, 32, False),
    (96, 160, 64, -10, 5, False), (96, 160, 64, 130, 5, False), (96, 160, 64, 40, -50, False), (96, 160, 64, 40, 80, False),
    (96, 160, 64, -63, -63, False), (96, 160, 64, 159, 95, False), (96, 160, 64, -64, 0, False), (96, 160, 64, 160, 0, False),
    (96, 160, 8, 33, 49, False), (96, 160, 16, 32, 48, False), (96, 160, 1, 159, 95, False),
    (96, 160, 64, 130, 5, True), (96, 160, 64, 40, 80, True), (96, 160, 64, 150, 90, True), (96, 160, 64, -10, -10, True),
    (96, 160, 64, 160 * 5 + 3, -96 * 7 - 2, True),
    (64, 64, 64, 0, 0, True), (64, 64, 64, 8, 0, True), (64, 64, 64, 5, 59, True),
    (64, 72, 64, 0, 0, True), (64, 72, 64, 8, 0, True), (64, 72, 64, 12, 3, True), (72, 64, 64, 3, 12, True), (72, 72, 64, 12, 12, True),
    (90, 150, 64, 100, 40, False), (90, 150, 64, 86, 26, False), (90, 150, 64, 140, 80, True), (90, 150, 64, 144, 80, False),
    (90, 150, 10, 140, 80, False), (90, 150, 64, -3, 88, True),
]


@pytest.mark.parametrize("case", WINDOWS, ids=lambda c: "H{}_W{}_R{}_x{}_y{}_{}".format(*c[:5], "wrap" if c[5] else "clip"))
def test_window_tiles_equal_the_restatement(lib, case):
    from diffusiontexturepainting_amd import ops
    H, W, R, x, y, wrap = case
    want = journal_ref.window_tiles(H, W, R, x, y, wrap)
    got = ops.journal_window_tiles(H, W, R, x, y, wrap=wrap)
    assert got == want
    assert got == sorted(set(got)) and all(0 <= t < journal_ref.tile_count(H, W) for t in got)


def test_window_tiles_cases_are_what_they_claim():
    t = journal_ref.window_tiles
    assert t(96, 160, 8, 33, 49, False) == [3 * 10 + 2]                      # entirely on one tile
    assert t(96, 160, 64, -64, 0, False) == [] and t(96, 160, 64, 160, 0, False) == []
    assert len(t(64, 64, 64, 8, 0, True)) == 16                              # W = R: every tile, each once
    assert len(t(64, 72, 64, 12, 3, True)) == 20                             # W = R + 8: columns 12 .. 71 and 0 .. 3 share tile column 0
    assert journal_ref.tile_count(90, 150) == 60 and 59 in t(90, 150, 64, 140, 80, True)  # the partial corner tile


def test_window_tiles_refusals(lib):
    n = C.c_int(7)
    buf = (C.c_int * 4)()

    def refused(pattern, *args):
        assert lib.dtp_journal_window_tiles(*args) == 1
        assert re.search(pattern, lib.dtp_last_error().decode()), lib.dtp_last_error()

    refused("NULL", 96, 160, 64, 0, 0, 0, None, 0, None)
    refused("NULL", 96, 160, 64, 0, 0, 0, None, 4, C.byref(n))
    refused("0 x 160", 0, 160, 64, 0, 0, 0, buf, 4, C.byref(n))
    refused("32769", 96, 32769, 64, 0, 0, 0, buf, 4, C.byref(n))
    refused("R=0", 96, 160, 0, 0, 0, 0, buf, 4, C.byref(n))
    refused("R=97", 96, 160, 97, 0, 0, 0, buf, 4, C.byref(n))
    refused("16 tiles, room for 4", 96, 160, 64, 0, 0, 0, buf, 4, C.byref(n))
    assert n.value == 16 and list(buf) == [0, 0, 0, 0]  # the count needed; nothing written
    assert lib.dtp_journal_window_tiles(96, 160, 64, 0, 160, 0, None, 0, C.byref(n)) == 0 and n.value == 0  # outside: no tile, no error


# ---------------------------------------------------------------- refusals that need no device
def test_create_refuses_before_any_device_call(lib):
    tex = (C.c_uint8 * 64)()
    base = C.addressof(tex)
    base += (-base) % 4
    out = C.c_void_p()

    def refused(pattern, ctx, texture, H, W, cap, depth, outp=out):
        assert lib.dtp_journal_create(ctx, texture, H, W, cap, depth, C.byref(outp) if outp is not None else None) == 1
        assert re.search(pattern, lib.dtp_last_error().decode()), lib.dtp_last_error()
        assert not out.value

    refused("texture is NULL", None, None, 90, 150, 8, 10)
    refused(r"a 0 x 150 texture", None, base, 0, 150, 8, 10)
    refused(r"a 90 x 32769 texture", None, base, 90, 32769, 8, 10)
    refused(r"a -1 x 150 texture", None, base, -1, 150, 8, 10)
    refused("4-byte aligned", None, base + 1, 90, 150, 8, 10)
    refused("4-byte aligned", None, base + 2, 90, 150, 8, 10)
    refused("capacity_tiles=0", None, base, 90, 150, 0, 10)
    refused("capacity_tiles=-5", None, base, 90, 150, -5, 10)
    refused("depth=0", None, base, 90, 150, 8, 0)
    refused("depth=65", None, base, 90, 150, 8, 65)
    refused("out is NULL", None, base, 90, 150, 8, 10, outp=None)
    refused("ctx is NULL", None, base, 90, 150, 8, 10)  # every other argument is fine: only now is the handle looked at


def test_a_pointer_that_is_no_live_journal_is_refused_and_not_followed(lib):
    junk = (C.c_uint8 * 4096)(*([0xAB] * 4096))  # followed, these bytes would be pointers into nowhere
    p = C.c_void_p(C.addressof(junk))
    rect = (C.c_int * 4)(0, 0, 5, 5)
    a, b, o, h = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_uint64(99)
    n = C.c_int(-1)
    calls = {
        "dtp_journal_begin": lambda q: lib.dtp_journal_begin(q, None),
        "dtp_journal_end": lambda q: lib.dtp_journal_end(q, None),
        "dtp_journal_touch": lambda q: lib.dtp_journal_touch(q, rect, 1, None),
        "dtp_journal_undo": lambda q: lib.dtp_journal_undo(q, None),
        "dtp_journal_redo": lambda q: lib.dtp_journal_redo(q, None),
        "dtp_journal_info": lambda q: lib.dtp_journal_info(q, C.byref(a), C.byref(b), C.byref(o), C.byref(h)),
        "dtp_journal_record_info": lambda q: lib.dtp_journal_record_info(q, 0, None, None, None),
        "dtp_op_journal_tiles": lambda q: lib.dtp_op_journal_tiles(q, 0, rect, 4, C.byref(n)),
    }
    for name, call in calls.items():
        assert call(p) == 1, name
        assert re.search(rf"{name}: not a live journal", lib.dtp_last_error().decode()), lib.dtp_last_error()
        assert call(None) == 1, name
        assert re.search(rf"{name}: the journal is NULL", lib.dtp_last_error().decode()), lib.dtp_last_error()
    assert (a.value, b.value, o.value, h.value, n.value) == (-1, -1, -1, 99, -1)
    assert lib.dtp_journal_destroy(p) == 1 and b"not a live journal" in lib.dtp_last_error()
    assert lib.dtp_journal_destroy(None) == 0  # a no-op
    assert bytes(junk) == b"\xab" * 4096


def test_touch_names_the_bad_rectangle(lib):
    junk = (C.c_uint8 * 64)()
    p = C.c_void_p(C.addressof(junk))

    def refused(pattern, rects, n):
        arr = (C.c_int * max(len(rects), 1))(*rects) if rects is not None else None
        assert lib.dtp_journal_touch(p, arr, n, None) == 1
        assert re.search(pattern, lib.dtp_last_error().decode()), lib.dtp_last_error()

    refused("rects is NULL", None, 1)
    refused(r"n=0 rectangles", [0, 0, 1, 1], 0)
    refused(r"n=-2 rectangles", [0, 0, 1, 1], -2)
    refused(r"rectangle 1 \(9, 0, 8, 0\) has x0 > x1", [0, 0, 5, 5, 9, 0, 8, 0], 2)
    refused(r"rectangle 0 \(0, 3, 0, 2\) has x0 > x1 or y0 > y1", [0, 3, 0, 2], 1)
    refused(r"rectangle 2 ", [0, 0, 0, 0, 1, 1, 1, 1, 5, 5, 4, 5], 3)


# ---------------------------------------------------------------- the restatement itself
def test_restatement_records_cursor_depth_and_ring():
    r = journal_ref.Records(capacity=10, depth=2)
    sizes = []
    for n in (4, 3, 5):  # three records at depth 2: the first goes
        r.begin()
        sizes.append(len(r.take(n)))
        r.end()
    assert r.head == 12 and r.records == [[4, 7], [7, 12]] and r.cursor == 2
    assert r.restorable(0) and r.restorable(1)
    assert r.undo() == [7, 12] and r.undo() == [4, 7] and r.undo() is None
    assert r.redo() == [4, 7] and r.cursor == 1
    r.begin()  # drops the undone record; head is not rewound
    assert r.records == [[4, 7], [12, 12]] and r.cursor == 2
    with pytest.raises(RuntimeError, match="open"):
        r.undo()
    r.take(3)
    r.end()
    assert r.head == 15 and not r.restorable(0) and r.restorable(1)  # 15 - 4 > 10
    assert r.undo() == [12, 15]
    with pytest.raises(RuntimeError, match="overwritten"):
        r.undo()
    assert r.records == [[12, 15]] and r.cursor == 0 and r.redo() == [12, 15]
    big = journal_ref.Records(capacity=3, depth=10)
    big.begin(); big.take(4); big.end()
    with pytest.raises(RuntimeError, match="overwritten"):
        big.undo()
    assert big.records == []


def test_restatement_journal_undoes_and_redoes_bytes():
    rng = np.random.default_rng(5)
    tex = rng.integers(0, 256, (90, 150, 4), dtype=np.uint8)
    states = [tex.copy()]
    j = journal_ref.Journal(tex, capacity=200, depth=10)
    for rect in [(140, 80, 149, 89), (0, 0, 149, 89), (17, 3, 40, 20)]:
        j.begin()
        new = j.touch([rect, rect])
        assert set(new) == journal_ref.rect_tiles(90, 150, rect) and len(new) == len(set(new))
        assert j.touch([rect]) == []  # once per record
        tex[rect[1]:rect[3] + 1, rect[0]:rect[2] + 1] = rng.integers(0, 256, (rect[3] - rect[1] + 1, rect[2] - rect[0] + 1, 4), dtype=np.uint8)
        j.end()
        states.append(tex.copy())
    assert j.rec.head == 2 + 60 + 4  # the corner's two partial tiles, every tile, a rectangle that straddles four
    for k in (2, 1, 0):
        assert j.undo() and np.array_equal(tex, states[k])
    assert not j.undo()
    for k in (1, 2, 3):
        assert j.redo() and np.array_equal(tex, states[k])
    assert not j.redo()


# ---------------------------------------------------------------- the stand-alone host program
def test_host_check_program_builds_and_passes(tmp_path):
    """tools/journal_host_check.cpp drives csrc/journal_host.h from its own main().  Here it is built plainly and run; the sanitizer run is
    the same program, built and run by hand (never from pytest, never with a preload):
        c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I diffusiontexturepainting_amd/csrc \\
            tools/journal_host_check.cpp -o journal_host_check && ./journal_host_check
    """
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "journal_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "diffusiontexturepainting_amd", "csrc"),
                        os.path.join(ROOT, "tools", "journal_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "checks passed" in r.stdout, r.stdout + r.stderr
