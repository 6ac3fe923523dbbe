"""The C-ABI library loads without a GPU and exports every symbol include/*.h declares; without a device it fails
loudly (there is no CPU fallback in the product)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


HEADERS = ("brs.h", "brs_policy.h", "brs_render.h", "brs_qpolicy.h")


def _declared(header):
    """{function name: number of parameters} of every function the header declares"""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {name: 0 if params.strip() in ("", "void") else params.count(",") + 1
            for name, params in re.findall(r"\b(brs_[a-z_0-9]+)\s*\(([^()]*)\)", txt)}


def test_header_symbols_exported():
    """one table (_lib.SIGNATURES) holds the C ABI: every function a header declares has an entry under that header with
    as many arguments as the declaration, every entry is declared, exported and applied, and the symbol lists derive from it"""
    from balance_robot_mujoco_rl_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert sorted(_lib.SIGNATURES) == sorted(HEADERS)
    for header in HEADERS:
        declared, table = _declared(header), _lib.SIGNATURES[header]
        assert sorted(declared) == sorted(table), (header, sorted(set(declared) ^ set(table)))
        for name, nparam in declared.items():
            restype, argtypes = table[name]
            assert hasattr(L, name), f"{name} declared in include/{header} but not exported by libbrs_hip.so"
            assert len(argtypes) == nparam, f"{name}: include/{header} declares {nparam} parameters, the table {len(argtypes)}"
            fn = getattr(L, name)
            assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert len(_declared("brs.h")) + len(_declared("brs_policy.h")) >= 15
    assert sorted(_lib.SYMBOLS) == sorted(list(_declared("brs.h")) + list(_declared("brs_policy.h")))
    assert sorted(_lib.RENDER_SYMBOLS) == sorted(_declared("brs_render.h"))
    assert sorted(_lib.QPOLICY_SYMBOLS) == sorted(_declared("brs_qpolicy.h"))


def test_sizes_and_bad_args_without_device():
    from balance_robot_mujoco_rl_amd import _lib
    L = _lib.lib()
    nq, nv, no, na = (C.c_int32() for _ in range(4))
    assert L.brs_sizes(1, C.byref(nq), C.byref(nv), C.byref(no), C.byref(na)) == 0
    assert (nq.value, nv.value, no.value, na.value) == (9, 8, 6, 2)
    assert L.brs_sizes(3, C.byref(nq), C.byref(nv), None, None) == 0 and (nq.value, nv.value) == (16, 14)
    assert L.brs_sizes(7, None, None, None, None) == -1
    h = C.c_void_p()
    assert L.brs_create(None, C.byref(h)) == -1
    cfg = _lib.BrsConfig(9, 4, 0, 0, 0, 0, 0, 0, 0.0, 0, 0)
    assert L.brs_create(C.byref(cfg), C.byref(h)) == -1 and b"variant" in L.brs_last_error(None)
    cfg = _lib.BrsConfig(1, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, 0)
    assert L.brs_create(C.byref(cfg), C.byref(h)) == -1
    cfg = _lib.BrsConfig(1, 8, 0, 6, 0, 0, 0, 0, 0.0, 0, 0)  # NOISE_ON | NOISE_OFF
    assert L.brs_create(C.byref(cfg), C.byref(h)) == -1
    # include/brs_policy.h: argument checks that need no device
    assert L.brs_policy_create(0, None) == -1
    assert L.brs_gae(0, 0, 4, None, None, None, None, None, 0.99, 0.95, None, None, None) == -1


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the loud-failure path is for machines without one")
    from balance_robot_mujoco_rl_amd import BatchedSim, BrsError, _lib
    with pytest.raises(BrsError):
        BatchedSim("Env01-v2", 4)
    L = _lib.lib()
    h = C.c_void_p()
    cfg = _lib.BrsConfig(1, 8, 0, 0, 0, 0, 0, 0, 0.0, 0, 0)
    assert L.brs_create(C.byref(cfg), C.byref(h)) == -2  # BRS_ERR_HIP
    assert b"no CPU fallback" in L.brs_last_error(None)


def test_every_family_fails_loudly_without_a_device():
    """all three handle families go through the same device check (csrc/brs_host.hpp): BRS_ERR_HIP, and each family's
    handle-less error text says that there is no CPU fallback"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the loud-failure path is for machines without one")
    from balance_robot_mujoco_rl_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    cfg = _lib.BrsConfig(3, 65, 0, 0, 0, 0, 0, 0, 0.0, 0, 0)
    for create, last_error, who in ((lambda: L.brs_create(C.byref(cfg), C.byref(h)), L.brs_last_error, b"brs_create"),
                                    (lambda: L.brs_policy_create(0, C.byref(h)), L.brs_policy_last_error, b"brs_policy_create"),
                                    (lambda: L.brs_qpolicy_create(0, C.byref(h)), L.brs_qpolicy_last_error, b"brs_qpolicy_create")):
        assert create() == -2 and h.value is None, who   # BRS_ERR_HIP
        msg = last_error(None)
        assert msg.startswith(who + b": no HIP device (") and msg.endswith(b"); there is no CPU fallback"), msg
    # the slots are per family: the last failure of one is not overwritten by another's
    assert L.brs_create(None, C.byref(h)) == -1 and b"null argument" in L.brs_last_error(None)
    assert b"no CPU fallback" in L.brs_policy_last_error(None) and b"no CPU fallback" in L.brs_qpolicy_last_error(None)


def test_render_reports_a_bad_ordinal_as_an_argument_error():
    """with or without a device: brs_render has no handle, and an ordinal this machine does not have is BRS_ERR_ARG"""
    from balance_robot_mujoco_rl_amd import _lib
    L = _lib.lib()
    cam = _lib.BrsCamera(); L.brs_render_default_camera(C.byref(cam))
    buf = C.c_void_p(1)
    for ordinal in (-1, 1 << 20):
        assert L.brs_render(ordinal, 3, 1, buf, C.byref(cam), buf, None, None, None) == -1
        assert L.brs_render_last_error() == b"brs_render: bad device ordinal"


def test_product_never_imports_oracle():
    """the product package must not reference oracle/ or the host test build"""
    pkg = os.path.join(ROOT, "balance_robot_mujoco_rl_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hpp", ".hip", ".h")):
                t = open(os.path.join(dp, f)).read()
                assert "import oracle" not in t and "from oracle" not in t and "libbrs_oracle" not in t, f
                assert "libbrs_hostsim" not in t, f


def test_tools_and_entry_points_compile():
    """every script under tools/ and the driver entry points are at least syntactically valid Python (most of them only
    run on a GPU box)"""
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = glob.glob(os.path.join(root, "tools", "*.py")) + [os.path.join(root, f) for f in ("bench.py", "__graft_entry__.py")]
    assert len(files) >= 8
    for f in files:
        compile(open(f).read(), f, "exec")
