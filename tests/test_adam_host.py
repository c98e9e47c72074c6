"""cgcn_adam_step (ABI v26), CPU side: declared in the header, bound by _lib, its host-side argument checks return the
documented codes without launching anything, and torch.ops.chromegcn.adam_step_ is registered with a fake implementation."""
import ctypes
import os
import re

import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from chromegcn_amd import _build, _lib
from chromegcn_amd import torch_ops  # noqa: F401  (registers the operators)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -1, -2


def test_header_declares_it_and_the_binding_has_it():
    src = open(os.path.join(ROOT, "include", "chromegcn.h")).read()
    assert re.search(r"#define CGCN_ABI_VERSION 26\b", src)
    m = re.search(r"int cgcn_adam_step\(([^)]*)\);", src)
    assert m, "cgcn_adam_step is not declared"
    assert len(m.group(1).split(",")) == 16
    assert "cgcn_adam_step" in _lib.exported_symbols()
    res, args = _lib._SIGNATURES["cgcn_adam_step"]
    assert res is ctypes.c_int and len(args) == 16
    assert _lib.ABI_VERSION == 26


def test_library_reports_abi_26_and_checks_arguments_on_the_host():
    _build.build_library()
    lib = _lib.load()
    assert lib.cgcn_abi_version() == 26
    # fake, 16-byte-aligned "device" addresses: every call below must be refused before anything is launched
    P, G, M, V, S, T = (0x10000 * k for k in range(1, 7))

    def call(count=1024, p=P, g=G, m=M, v=V, s=S, n_step=4, t=T, lr=1e-3, b1=0.9, b2=0.98, eps=1e-8, wd=0.0, gs=1.0):
        return lib.cgcn_adam_step(None, count, p, g, m, v, s, n_step, t, lr, b1, b2, eps, wd, gs, None)

    assert call(count=-1) == BAD_ARG
    assert call(count=1 << 31) == UNSUPPORTED
    assert call(n_step=0) == BAD_ARG and call(n_step=-3) == BAD_ARG
    assert call(s=None) == BAD_ARG and call(t=None) == BAD_ARG
    for kw in ("p", "g", "m", "v"):
        assert call(**{kw: None}) == BAD_ARG, kw
        assert call(**{kw: P + 4}) == BAD_ARG, kw          # not 16-byte aligned
    for b1, b2 in ((1.0, 0.98), (-0.1, 0.98), (0.9, 1.0), (0.9, -1e-3), (float("nan"), 0.98), (0.9, float("nan"))):
        assert call(b1=b1, b2=b2) == BAD_ARG, (b1, b2)
    assert call(eps=-1e-8) == BAD_ARG and call(eps=float("nan")) == BAD_ARG


def test_operator_is_registered_and_its_fake_runs():
    op = torch.ops.chromegcn.adam_step_
    s = str(op.default._schema)
    for name in ("param", "exp_avg", "exp_avg_sq", "step", "ticket"):
        assert re.search(r"Tensor\(a\d+!\) %s\b" % name, s), (name, s)
    assert "-> ()" in s
    with FakeTensorMode():
        p = torch.empty(1000, device="cuda")
        step = torch.zeros(5, device="cuda")
        ticket = torch.zeros(1, device="cuda", dtype=torch.int32)
        assert op(p, p.clone(), p.clone(), p.clone(), step, ticket, 1e-3, 0.9, 0.98, 1e-8, 0.0, 1.0, None) is None
