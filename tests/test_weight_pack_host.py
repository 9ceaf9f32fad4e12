"""CPU: the selection and the argument checks of the device-side weight packs (csrc/weight_pack.hip, ops.pack_*_device, arith.Arith.device_packs).

What runs on the GPU is tests/test_gpu_weight_pack.py.  Here: the flag is off by default and parses from the environment, no decision of
unet3d.conv_plan depends on it (every case and arithmetic of tests/unet_dispatch_cases.py), the builders refuse by name before the library is loaded,
the C entries refuse by return code before any launch (the pointers are numbers that are never followed), and _lib's signatures match the header."""
import ctypes
import os
import re

import pytest
import torch

from garmentnets_amd import _lib, arith as AR, ops
from garmentnets_amd.arith import SPLIT_BF16X3, SPLIT_F16X2, Arith
import unet_dispatch_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gn_weight_pack_split", "gn_weight_pack_split_wino", "gn_weight_pack_upconv")
SIZES = ("gn_weight_pack_split_bytes", "gn_weight_pack_split_wino_bytes", "gn_weight_pack_upconv_bytes")
CTYPE = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}


def test_off_by_default():
    assert Arith().device_packs is False
    assert Arith().replace(device_packs=True).device_packs is True
    assert Arith().replace(device_packs=True) != Arith()
    assert Arith().strict_fp32().device_packs is False and Arith(device_packs=True).strict_fp32().device_packs is True


@pytest.mark.parametrize("value, expected", [(None, False), ("0", False), ("1", True)])
def test_environment_flag(monkeypatch, value, expected):
    if value is None:
        monkeypatch.delenv("GARMENTNETS_DEVICE_PACKS", raising=False)
    else:
        monkeypatch.setenv("GARMENTNETS_DEVICE_PACKS", value)
    a = Arith.from_env()
    assert a.device_packs is expected
    assert a.replace(device_packs=False) == Arith.from_env().replace(device_packs=False)      # (nothing else moves with it)
    assert "device_packs" in AR.__doc__


@pytest.mark.parametrize("arith_name", sorted(C.ARITHS))
@pytest.mark.parametrize("case", sorted(C.CASES))
def test_conv_plan_does_not_depend_on_it(monkeypatch, case, arith_name):
    B = C.CASES[case]["B"]
    off = C.plan_walk(case, arith_name, B)
    monkeypatch.setattr(C, "arith", lambda name: Arith(**C.ARITHS[name]).replace(device_packs=True))
    assert C.arith(arith_name).device_packs is True
    on = C.plan_walk(case, arith_name, B)
    assert len(off) > 0 and on == off


def _no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "call", refuse)


def test_builders_refuse_a_cpu_tensor_before_loading(monkeypatch):
    _no_library(monkeypatch)
    w = torch.zeros(32, 32, 3, 3, 3)
    with pytest.raises(ValueError, match="pack_conv_weight_split_device.*GPU"):
        ops.pack_conv_weight_split_device(w, SPLIT_F16X2)
    with pytest.raises(ValueError, match="pack_conv_weight_split_wino_device.*GPU"):
        ops.pack_conv_weight_split_wino_device(w)
    with pytest.raises(ValueError, match="pack_upconv_weight_device.*GPU"):
        ops.pack_upconv_weight_device(w, 16, SPLIT_F16X2)


def _cpu(shape, dtype=torch.float32, contiguous=True):
    t = torch.zeros(shape, dtype=dtype)
    return t if contiguous else t.permute(0, 1, 4, 3, 2)


def test_builders_refuse_bad_widths_before_loading(monkeypatch):
    _no_library(monkeypatch)
    weight = _cpu
    for shape, kw, what in (((32, 24, 3, 3, 3), {}, "multiples of 16"), ((48, 32, 3, 3, 3), {}, "multiples of 16"),
                            ((32, 32, 3, 3, 3), dict(c_lo=16, c_n=32), "outside the weight"), ((32, 32, 3, 3, 3), dict(c_lo=0, c_n=8), "multiples of 16"),
                            ((32, 32, 3, 3, 1), {}, "Conv3d weight")):
        with pytest.raises(ValueError, match=what):
            ops.pack_conv_weight_split_device(weight(shape), SPLIT_F16X2, **kw)
        with pytest.raises(ValueError, match=what):
            ops.pack_conv_weight_split_wino_device(weight(shape), **kw)
    for shape, c0, what in (((32, 48, 3, 3, 3), 40, "multiples of 16"), ((48, 48, 3, 3, 3), 32, "multiples of 16"), ((32, 48, 3, 3, 3), 48, "outside the weight"),
                            ((32, 48, 3, 3, 3), -16, "outside the weight")):
        with pytest.raises(ValueError, match=what):
            ops.pack_upconv_weight_device(weight(shape), c0, SPLIT_F16X2)
    with pytest.raises(ValueError, match="float32"):
        ops.pack_conv_weight_split_device(weight((32, 32, 3, 3, 3), dtype=torch.float16), SPLIT_F16X2)
    with pytest.raises(ValueError, match="contiguous"):
        ops.pack_conv_weight_split_wino_device(weight((32, 32, 3, 3, 3), contiguous=False))
    with pytest.raises(ValueError, match="unknown split mode"):
        ops.pack_conv_weight_split_device(weight((32, 32, 3, 3, 3)), 7)
    with pytest.raises(ValueError, match="two-plane"):
        ops.pack_upconv_weight_device(weight((32, 48, 3, 3, 3)), 32, SPLIT_BF16X3)


def _declaration(hdr, name):
    m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/garmentnets_hip.h"
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        args.append(ctypes.c_void_p if "*" in a else CTYPE[a.replace("const ", "").split()[0]])
    return CTYPE[m.group(1)], args


def test_signatures_are_the_headers():
    hdr = open(os.path.join(REPO, "include", "garmentnets_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES + SIZES:
        res, args = _declaration(hdr, name)
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
        assert _lib.PROTOTYPES[name] == args, name
        assert _lib._RESTYPES.get(name, ctypes.c_int) is res, name
    make = open(os.path.join(REPO, "garmentnets_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bweight_pack\.hip\b", make, re.M)


def test_sizes():
    lib = _lib.load()
    assert lib.gn_weight_pack_split_bytes(16, 32, SPLIT_F16X2) == (27 + 8) * 2 * 1024
    assert lib.gn_weight_pack_split_bytes(48, 96, SPLIT_BF16X3) == (3 * 27 + 8) * 3 * 3 * 1024
    assert lib.gn_weight_pack_split_wino_bytes(48, 96) == (3 * 36 + 6) * 3 * 2 * 1024
    assert lib.gn_weight_pack_upconv_bytes(16, 32) == 64 * 2 * 1024
    assert lib.gn_weight_pack_split_bytes(24, 32, SPLIT_F16X2) == 0 and lib.gn_weight_pack_split_bytes(16, 48, SPLIT_F16X2) == 0
    assert lib.gn_weight_pack_split_bytes(16, 32, 7) == 0 and lib.gn_weight_pack_split_wino_bytes(8, 32) == 0 and lib.gn_weight_pack_upconv_bytes(16, 16) == 0


def test_entries_refuse_by_return_code():
    """GN_EINVAL before any launch: c_n % 16, Cout % 32, a range outside the weight, an unknown mode, a short or misaligned pack"""
    lib, vp, big = _lib.load(), ctypes.c_void_p, 1 << 30

    def split(cout=32, cin=32, c_lo=0, c_n=32, mode=SPLIT_F16X2, pack=0x2000, nbytes=big):
        return lib.gn_weight_pack_split(vp(0x1000), cout, cin, c_lo, c_n, mode, vp(pack), nbytes, vp(0x3000), None)

    def wino(cout=32, cin=32, c_lo=0, c_n=32, pack=0x2000, nbytes=big):
        return lib.gn_weight_pack_split_wino(vp(0x1000), cout, cin, c_lo, c_n, vp(pack), nbytes, vp(0x3000), None)

    def upconv(cout=32, cin=48, c0=32, mode=SPLIT_F16X2, pack=0x2000, nbytes=big):
        return lib.gn_weight_pack_upconv(vp(0x1000), cout, cin, c0, mode, vp(pack), nbytes, vp(0x3000), None)

    for fn in (split, wino):
        for kw, what in ((dict(c_n=24), "multiples of 16"), (dict(cout=48), "multiples of 16"), (dict(c_lo=16), "outside the weight"),
                         (dict(c_lo=-16), "outside the weight"), (dict(nbytes=1024), "too small"), (dict(pack=0x2008), "16-byte aligned")):
            assert fn(**kw) == _lib.GN_EINVAL, (fn.__name__, kw)
            assert what in lib.gn_last_error().decode(), (fn.__name__, kw, lib.gn_last_error().decode())
    for mode in (0, 1, 5, -1):
        assert split(mode=mode) == _lib.GN_EINVAL and "unknown split mode" in lib.gn_last_error().decode()
    for kw, what in ((dict(c0=40), "multiples of 16"), (dict(cout=48), "multiples of 16"), (dict(c0=48), "split point"), (dict(c0=-16), "split point"),
                     (dict(mode=SPLIT_BF16X3), "two-plane"), (dict(nbytes=1024), "too small")):
        assert upconv(**kw) == _lib.GN_EINVAL, kw
        assert what in lib.gn_last_error().decode(), (kw, lib.gn_last_error().decode())


def test_training_command_line_selects_it():
    from garmentnets_amd import train_pipeline as TP
    assert TP.parse_args(["--zarr_in", "x.zarr"]).host_packs is False
    assert TP.parse_args(["--zarr_in", "x.zarr", "--host_packs"]).host_packs is True
