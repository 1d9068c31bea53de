"""The C-ABI library builds for gfx950, loads, and exports every symbol include/vl3d.h declares (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from videoloop3d_amd import _lib
    return _lib


def header_symbols():
    src = open(os.path.join(ROOT, "include", "vl3d.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vl3d_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported(built):
    syms = header_symbols()
    assert len(syms) >= 15
    l = ctypes.CDLL(built.LIB_PATH)
    for s in syms:
        assert hasattr(l, s), f"{s} declared in include/vl3d.h but not exported"


def test_binding_covers_header(built):
    assert sorted(built.SIGNATURES) == header_symbols()


def test_no_gpu_calls_needed_for_metadata(built):
    assert built.lib().vl3d_version() >= 100


def test_struct_layout_matches_header(built):
    # 25 x 4-byte fields / (10 x 4 + pad + 6 x 8 + 4 + pad): catches accidental drift between vl3d.h and ctypes
    assert ctypes.sizeof(built.RenderDesc) == 104
    assert ctypes.sizeof(built.LossDesc) == 96
    assert ctypes.sizeof(built.Stage1ObjectiveDesc) == 64      # 4 x int32 + 12 x float
    assert ctypes.sizeof(built.BakedFrames) == 24              # 2 x int32 + 2 pointers
    assert ctypes.sizeof(built.BakedOut) == 40                 # 3 pointers + int32 + pad + pointer
    assert ctypes.sizeof(built.BwdChoice) == 40                # 10 x int32


def test_bwd_choice_fields_match_header(built):
    """vl3d_bwd_choice is written by the library into the caller's buffer: the binding has the header's fields, all int32, in the header's order"""
    src = open(os.path.join(ROOT, "include", "vl3d.h")).read()
    body = re.search(r"typedef struct vl3d_bwd_choice \{(.*?)\} vl3d_bwd_choice;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert all(d.startswith("int32_t ") for d in decls)
    names = [n.strip() for d in decls for n in d[len("int32_t "):].split(",")]
    assert names == [n for n, _ in built.BwdChoice._fields_] and len(names) == 10
    assert all(t is ctypes.c_int32 for _, t in built.BwdChoice._fields_)


def test_cpu_tensor_is_rejected_loudly(built):
    import torch
    from videoloop3d_amd.render import render_planes
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render_planes(torch.zeros(2, 1, 8, 8, 4), torch.eye(3).expand(2, 3, 3), 8, 8)


def test_a_library_built_from_other_sources_is_refused(tmp_path):
    """__graft_entry__.build() stamps the library with the sha256 of its sources; _lib refuses a library whose stamp names other sources (a stale
    prebuilt .so beside edited kernels would otherwise answer with old code behind unchanged symbols) and build() recompiles instead of trusting it."""
    import pytest
    import __graft_entry__ as ge
    from videoloop3d_amd import _lib as L
    ge.build()
    assert open(ge.STAMP).read().strip() == ge.source_hash() == L.sources_sha256()
    L.check_stamp(ge.LIB)                                           # the tree's own library passes
    (tmp_path / "libvl3d_hip.stamp").write_text("0" * 64 + "\n")
    with pytest.raises(RuntimeError, match="other sources"):
        L.check_stamp(str(tmp_path / "libvl3d_hip.so"))
