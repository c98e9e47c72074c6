"""The named parameter table of chromegcn_amd/_lib.py and its keyword call path (no GPU needed): the table matches
include/chromegcn.h name for name and type for type, the call path hands every argument to the C function in header
order, and no module of the package calls the library around it."""
import ctypes
import glob
import os
import re

import pytest
import torch

from chromegcn_amd import _build, _lib

from test_cabi_symbols import ROOT, declared_symbols

# C type -> ctypes type of the binding; every other `T *` is a c_void_p
_SCALARS = {"int": ctypes.c_int, "unsigned int": ctypes.c_uint, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "cgcn_stream_t": ctypes.c_void_p}
_RESULTS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "void": None, "const char *": ctypes.c_char_p}
# the pointer-to-result parameters bound as typed pointers
_TYPED_POINTERS = {"size_t *": ctypes.POINTER(ctypes.c_size_t)}


def header_prototypes():
    """{name: (return type, [(parameter name, C type), ...])} of every function include/chromegcn.h declares"""
    src = open(os.path.join(ROOT, "include", "chromegcn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"^([A-Za-z_][\w \*]*?)\b(cgcn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, re.M):
        params = " ".join(m.group(3).split())
        plist = []
        for p in ([] if params == "void" else params.split(",")):
            ctype, name = re.match(r"\s*(.*?)\s*(\w+)\s*$", p).groups()
            plist.append((name, " ".join(ctype.replace("*", " *").split())))
        protos[m.group(2)] = (" ".join(m.group(1).replace("*", " *").split()), plist)
    return protos


def _ctypes_of(ctype):
    if ctype in _TYPED_POINTERS:
        return _TYPED_POINTERS[ctype]
    return ctypes.c_void_p if ctype.endswith("*") else _SCALARS[ctype.replace("const ", "")]


def test_table_matches_the_header_names_types_and_order():
    protos = header_prototypes()
    assert sorted(protos) == declared_symbols() == sorted(_lib._ABI)
    for fn, (ret, params) in protos.items():
        res, table = _lib._ABI[fn]
        assert res is _RESULTS[ret], fn
        assert [p for p, _ in table] == [p for p, _ in params], fn
        assert [t for _, t in table] == [_ctypes_of(c) for _, c in params], fn
        assert _lib._SIGNATURES[fn] == (res, [t for _, t in table]), fn


class _Recorder:
    """stands in for the loaded library: every function records its positional arguments and returns 0"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, fn):
        return lambda *args: self.calls.append((fn, args)) or 0


def test_every_entry_point_gets_its_arguments_in_header_order(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "_lib", rec)
    for fn, (_, params) in _lib._ABI.items():
        sentinels = {p: 1000 + i for i, (p, _) in enumerate(params)}
        assert _lib.query(fn, **dict(reversed(list(sentinels.items())))) == 0
        assert rec.calls[-1] == (fn, tuple(sentinels.values())), fn


def test_stream_defaults_to_torchs_and_pointers_are_converted(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "_lib", rec)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0xABC)
    t = torch.zeros(8)
    hg = _lib.HeadGrad()
    names = [p for p, _ in _lib._ABI["cgcn_layer_bwd"][1] if p != "stream"]
    args = dict.fromkeys(names, 7)
    args.update(X=t, dXn=None, head=hg, aux_t=t.data_ptr() + 16)
    _lib.call("cgcn_layer_bwd", **args)
    got = dict(zip(["stream"] + names, rec.calls[-1][1]))
    assert got["stream"] == 0xABC and got["X"] == t.data_ptr() and got["dXn"] is None and got["aux_t"] == t.data_ptr() + 16
    assert ctypes.addressof(got["head"]._obj) == ctypes.addressof(hg)    # a struct goes by reference
    out = ctypes.c_size_t()
    _lib.call("cgcn_head_workspace_layout", n=1, S=1, d=128, C=1, dym_offset=out, bnc_offset=out, part_offset=out)
    assert rec.calls[-1][1][4]._obj is out                                # so does an out-parameter
    _lib.call("cgcn_sddmm", stream=None, n=1, S=1, d=128, rowptr=t, col=t, A=t, B=t, out=t, accumulate=0)
    assert rec.calls[-1][1][0] is None                                    # a stream the caller gives is kept, NULL too


def test_missing_and_unknown_arguments_raise(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "_lib", rec)
    full = {p: 1 for p, _ in _lib._ABI["cgcn_sgd_step"][1]}
    missing = dict(full)
    del missing["momentum_buf"]
    with pytest.raises(TypeError, match="momentum_buf"):
        _lib.call("cgcn_sgd_step", **missing)
    with pytest.raises(TypeError, match="missing argument momentum_buf"):   # a misspelt name does not stand in for it
        _lib.call("cgcn_sgd_step", momentum_bufs=None, **missing)
    with pytest.raises(TypeError, match="unknown argument.*extra"):
        _lib.call("cgcn_sgd_step", extra=1, **full)
    assert rec.calls == []


def test_failures_of_the_real_library_raise_with_its_message():
    _build.build_library()
    _lib.load()
    args = dict(stream=None, count=1024, param=None, grad=0x20000, exp_avg=0x30000, exp_avg_sq=0x40000, step=0x50000,
                n_step=4, ticket=0x60000, lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-8, weight_decay=0.0, grad_scale=1.0,
                rng_state=None)
    with pytest.raises(RuntimeError, match=r"chromegcn_amd: cgcn_adam_step failed: bad argument.*\(code -1\)"):
        _lib.call("cgcn_adam_step", **args)
    assert _lib.query("cgcn_head_workspace_bytes", n=5000, S=3, d=128, C=5) == 0
    with pytest.raises(RuntimeError, match="unsupported shape"):
        _lib.head_workspace(5000, 3, 128, 5, "cpu")
    with pytest.raises(RuntimeError, match="unsupported shape"):
        _lib.layer_bwd_workspace(5000, 2, 100, "cpu")
    assert _lib.layer_bwd_workspace(40, 2, 128, "cpu").numel() == _lib.query("cgcn_layer_bwd_workspace_bytes", n=40, S=2, d=128)


def test_no_module_calls_the_library_around_the_table():
    for path in glob.glob(os.path.join(ROOT, "chromegcn_amd", "*.py")):
        if os.path.basename(path) != "_lib.py":
            src = open(path).read()
            assert not re.search(r"\.cgcn_\w+\s*\(", src), path
