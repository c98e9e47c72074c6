"""The label-pair ablation entry points (additions to ABI 26), CPU side: declared in the header, bound by _lib, the workspace
query answers and the host-side argument checks return the documented codes without launching anything."""
import os
import re

from chromegcn_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -1, -2
NAMES = ("cgcn_ablation_prepare", "cgcn_ablation_workspace_bytes", "cgcn_ablation_layer", "cgcn_ablation_head",
         "cgcn_ablation_mask", "cgcn_ablation_reduce")
P = 0x10000   # a fake, aligned "device" address: every call below is refused (or has nothing to do) before any launch


def test_declared_additively_in_abi_26():
    src = open(os.path.join(ROOT, "include", "chromegcn.h")).read()
    assert re.search(r"#define CGCN_ABI_VERSION 26\b", src)
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, src), name
        assert name in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 26


def test_workspace_query():
    _build.build_library()
    lib = _lib.load()
    q = lib.cgcn_ablation_workspace_bytes
    feat = 1000 * 2 * 128 * 4
    assert q(1000, 2, 128, 1) == feat + 4096
    assert q(1000, 2, 128, 2) == 2 * feat + 4096
    assert q(1000, 2, 256, 2) == 4 * feat + 4096
    assert q(3, 2, 128, 1) == 3072 + 256            # every part on a 256-byte boundary
    assert q(0, 2, 128, 2) == 0 + 0 + 0
    for args in ((10, 1, 128, 2), (10, 2, 64, 2), (10, 2, 128, 3), (10, 2, 128, 0), (-1, 2, 128, 2)):
        assert q(*args) == 0, args


def test_argument_checks_answer_without_launching():
    _build.build_library()
    lib = _lib.load()

    def layer(n=100, S=2, d=128, rowptr=P, X=P, n_pos=4, n_cols=3, cols=P, X_inst=None, pos_rank=P, C=7):
        return lib.cgcn_ablation_layer(None, n, S, d, rowptr, P, None, None, X, X_inst, P, P, P, P, P, C, P, pos_rank, n_pos,
                                       cols, n_cols, P, None)

    assert layer(n=-1) == BAD_ARG and layer(n_pos=-1) == BAD_ARG and layer(n_cols=-2) == BAD_ARG and layer(C=0) == BAD_ARG
    assert layer(S=1) == UNSUPPORTED and layer(S=3) == UNSUPPORTED and layer(d=64) == UNSUPPORTED
    assert layer(rowptr=None) == BAD_ARG and layer(X=None) == BAD_ARG and layer(cols=None) == BAD_ARG
    assert layer(X_inst=P, pos_rank=None) == BAD_ARG
    assert layer(n_pos=101) == UNSUPPORTED
    assert layer(n_pos=0) == 0 and layer(n_cols=0) == 0      # nothing to do: no launch

    def head(S=2, d=128, label=-1, X=P, X_inst=None, base=P, M=None, removed=None, cols=None, C=7):
        return lib.cgcn_ablation_head(None, 100, S, d, C, X, X_inst, P, P, P, P, 1e-5, P, P, P, P, label, 4, cols, 3,
                                      removed, base, M)

    assert head(d=100) == UNSUPPORTED and head(S=1) == UNSUPPORTED
    assert head(base=None) == BAD_ARG and head(X=None) == BAD_ARG and head(label=7) == BAD_ARG
    assert head(label=2) == BAD_ARG                           # pair mode needs X_inst, cols, removed and M
    assert head(label=2, X_inst=P, cols=P, removed=P) == BAD_ARG

    assert lib.cgcn_ablation_prepare(None, -1, 7, P, P, P, P, P) == BAD_ARG
    assert lib.cgcn_ablation_prepare(None, 100, 0, P, P, P, P, P) == BAD_ARG
    assert lib.cgcn_ablation_prepare(None, 100, 7, None, P, P, P, P) == BAD_ARG
    assert lib.cgcn_ablation_prepare(None, 1 << 25, 103, P, P, P, P, P) == UNSUPPORTED

    assert lib.cgcn_ablation_mask(None, 100, 7, P, P, None, None, P, 0, 7, P, P, P) == BAD_ARG
    assert lib.cgcn_ablation_mask(None, 100, 7, P, P, None, None, P, -1, 2, P, P, P) == BAD_ARG
    assert lib.cgcn_ablation_mask(None, 100, 7, P, P, None, None, P, 0, 2, None, P, P) == BAD_ARG
    assert lib.cgcn_ablation_mask(None, 100, 7, P, P, None, None, P, 0, 2, P, P, None) == BAD_ARG

    assert lib.cgcn_ablation_reduce(None, 100, 1, 7, P, P, P, -1, 0, None, P, None) == UNSUPPORTED
    assert lib.cgcn_ablation_reduce(None, 100, 2, 7, P, P, P, 3, 9, P, P, P) == BAD_ARG
    assert lib.cgcn_ablation_reduce(None, 100, 2, 7, None, P, P, -1, 0, None, P, None) == BAD_ARG
    assert lib.cgcn_ablation_reduce(None, 100, 2, 7, P, P, P, 3, 1, None, P, P) == BAD_ARG
