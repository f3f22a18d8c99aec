"""CPU-side checks of the two-operand e4m3 ABI additions (no GPU): the two new kernel-level entry points are declared in include/dtp.h,
bound by _lib.SYMBOLS and exported by libdtp.so; dtp_gemm_desc grew at its end only; the ABI version is unchanged."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dtp_op_gemm_f8f8", "dtp_op_quant_e4m3")


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_new_entry_points_declared_bound_and_exported(lib):
    from diffusiontexturepainting_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dtp.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.dtp_abi_version() == 3


def test_gemm_desc_grew_at_the_end():
    from diffusiontexturepainting_amd import _lib
    names = [f[0] for f in _lib.GemmDesc._fields_]
    assert names[-8:] == ["A8", "lda8", "A2_8", "lda2_8", "C8", "ldc8", "c_scale", "a2_scale"]
    # the fields every existing caller uses keep their offsets
    assert names.index("Wfr") == len(names) - 9
    assert _lib.GemmDesc.A8.offset >= _lib.GemmDesc.Wfr.offset + C.sizeof(C.c_void_p)
