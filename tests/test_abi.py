"""prs_abi_check's refusals, the loud failure without a GPU, and the package's independence of the oracle (no GPU needed).  What the
header declares against what the library exports and the binding restates is tests/test_abi_layout.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import _lib
    return _lib


def test_abi_check_refuses_another_version_or_size(built):
    lib = built.load()
    # a client built against another header, or with a shorter parameter struct, is refused instead of read past
    sizes = [C.sizeof(built.StereoParams), C.sizeof(built.PcfParams), C.sizeof(built.AlignerParams), C.sizeof(built.AlignBatch)]
    assert lib.prs_abi_check(built.ABI_VERSION, *sizes) == 0
    assert lib.prs_abi_check(built.ABI_VERSION - 1, *sizes) < 0
    assert lib.prs_abi_check(built.ABI_VERSION, sizes[0], sizes[1], sizes[2] - 12, sizes[3]) < 0
    assert lib.prs_status_string(-1).decode().startswith("required")


def test_context_create_without_gpu_fails_loudly(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = built.load()
    h = C.c_void_p()
    rc = lib.prs_context_create(0, C.byref(h))
    assert rc < 0  # PRS_ERR_NO_DEVICE (or HIP error): never a silent CPU path
    from srrg2_proslam_amd import ops
    with pytest.raises(built.ProslamHipError):
        ops.Context(0)


def test_product_package_never_touches_the_oracle():
    """the oracle is test infrastructure: nothing under srrg2_proslam_amd/ may reference it"""
    pkg = os.path.join(ROOT, "srrg2_proslam_amd")
    bad = []
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp", ".hpp")) or fn == "Makefile":
                text = open(os.path.join(dirpath, fn), errors="ignore").read()
                if re.search(r"\boracle\b", text):
                    bad.append(os.path.relpath(os.path.join(dirpath, fn), ROOT))
    assert not bad, "product files mention the oracle: %s" % bad
