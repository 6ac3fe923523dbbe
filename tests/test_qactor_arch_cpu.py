"""The int8 off-policy actor at its second width set, 6 -> 256 -> 256 -> 2 (SB3's SAC default), without a GPU:
the kernel's own source (brs_qactor.hpp, the Widths256 instantiation compiled for the host by g++) against the independent
reference (tests/ref_qactor.py), a stand-alone program of it under the sanitizers, the conditions on the case set, the quantiser
with net_arch="sb3" (known answers, the inputs it accepts, its errors, its quality against the fp64 float network, the file round
trip), and the argument checks of the library at these widths through brs_qpolicy_actor_check_model.  Every comparison of the
integer path is exact.  The cases are tests/qactor_cases.py's at these widths (tests/qactor_arch_cases.py)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from balance_robot_mujoco_rl_amd import _lib  # noqa: E402
from balance_robot_mujoco_rl_amd import QuantActorModel, quantize_actor, unflatten_sac_actor  # noqa: E402
from tests import qactor_arch_cases as A  # noqa: E402
from tests import ref_qactor as R  # noqa: E402

K = A.K
OK, ERR_ARG, ERR_STATE = 0, -1, -3
HOST_DIR = os.path.join(ROOT, "tests", "qactorarchhost")
GXX = ["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "balance_robot_mujoco_rl_amd", "csrc")]

# max |action(int8) - action(fp64 float network)| over K.in_box_obs(4096) at [256, 256]: MEASURED on the quantiser as it stands
# (fp64, on the numpy reference), not derived, and gated at twice the measurement, as tests/test_qactor_cpu.py does
# and for its reason: the default calibration is the reference's three rows (two corners and the origin), so the number is the
# quantiser's and the calibration's, not the kernel's.  The PD law is the same law as at the reference widths, hence about the same
# 0.25 (one int8 step of its output pre-activation); the torch-initialised network is smaller here than there (0.435) because its
# outputs are: 256 inputs of U(+-1/16) on the last layer
MEASURED_MAX_ERR = {"pd": 0.25027, "sb3": 0.09989}


@pytest.fixture(scope="module")
def models():
    return A.all_models()


@pytest.fixture(scope="module")
def inputs():
    return np.concatenate([K.seeded_obs(4097), K.special_rows()])


@pytest.fixture(scope="module")
def reference(models, inputs):
    """ref_qactor.act of every model on the inputs, computed once"""
    return [R.act(model, inputs) for _, model in models]


# ------------------------------------------------------------------------- 1. host build of brs_qactor.hpp at [256, 256]
def _load_host(directory, widths):
    so = os.path.join(str(directory), f"libqactorarchhost_{widths}.so")
    subprocess.check_call(GXX + [f"-DQAH_WIDTHS={widths}", "-fPIC", "-shared", "-o", so, os.path.join(HOST_DIR, "qactorarchhost.cpp")])
    L = C.CDLL(so)
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    L.qah_build.argtypes = [C.POINTER(_lib.BrsQActorModel), vp, C.c_char_p, C.c_int]
    L.qah_act.argtypes = [vp, C.c_int, vp, vp, vp]
    L.qah_widths.argtypes = [ip, ip, ip, ip]
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _load_host(tmp_path_factory.mktemp("qactorarchhost"), "Widths256")


def host_build(H, model):
    cm, keep = K.c_model(model)
    image = np.zeros(H.qah_image_bytes() // 16 + 1, np.complex128)   # 16-byte elements: the image is alignas(16)
    err = C.create_string_buffer(256)
    rc = H.qah_build(C.byref(cm), image.ctypes.data, err, 256)
    return rc, err.value.decode(), image


def host_act(H, model, obs, want_q=True):
    rc, err, image = host_build(H, model)
    assert rc == 0, err
    obs = np.ascontiguousarray(obs, np.float32)
    a, q = np.full((obs.shape[0], 2), np.nan, np.float32), np.full((obs.shape[0], 2), 99, np.int8)
    H.qah_act(image.ctypes.data, obs.shape[0], obs.ctypes.data, a.ctypes.data, q.ctypes.data if want_q else None)
    return a, q


def test_the_instantiation_has_the_sizes_the_design_states(host, tmp_path):
    w = [C.c_int() for _ in range(4)]
    host.qah_widths(*[C.byref(v) for v in w])
    assert [v.value for v in w] == [256, 256, 256, 256], "no padded unit"
    assert host.qah_arch() == _lib.ARCH_SAC_DEFAULT == 1 and host.qah_image_bytes() == 80208
    ref = _load_host(tmp_path, "WidthsReference")
    ref.qah_widths(*[C.byref(v) for v in w])
    assert [v.value for v in w] == [300, 200, 320, 224] and ref.qah_arch() == 0 and ref.qah_image_bytes() == 86480
    # each instantiation refuses the other's model, and names its own network
    from tests import qactor_cases as K0
    for H, model, text in ((host, K0.random_model(0), "6-256-256-2"), (ref, K.random_model(0), "6-300-200-2")):
        rc, err, _ = host_build(H, model)
        assert rc == ERR_ARG and err == "brs_qpolicy_actor_set_model: layer 0: the network must be " + text


@pytest.mark.parametrize("which", range(17))
def test_host_build_equals_reference(host, models, inputs, reference, which):
    name, model = models[which]
    a_ref, q_ref = reference[which]
    a, q = host_act(host, model, inputs)
    assert np.array_equal(q, q_ref), f"{name}: {int((q != q_ref).any(axis=1).sum())} rows differ"
    assert np.array_equal(a, a_ref) and a.dtype == np.float32, name
    a2, q2 = host_act(host, model, inputs[:65], want_q=False)
    assert np.array_equal(a2, a_ref[:65]) and (q2 == 99).all(), "action_q = NULL"


def test_there_are_seventeen_models(models):
    assert len(models) == 17 and len({name for name, _ in models}) == 17
    assert all([L["W"].shape for L in m["layers"]] == [(256, 6), (256, 256), (2, 256)] for _, m in models)


@pytest.mark.parametrize("seed", range(3))
def test_random_models_do_not_collapse(inputs, seed):
    """tests/test_qactor_cpu.py's condition on the random models, on the reference alone: more than 50 distinct action codes, and
    more than 50 distinct codes behind each hidden layer; every tensor has a non-zero zero point.  (Measured at these widths: 69,
    140 and 108 action codes, at least 176 behind each hidden layer)"""
    model = K.random_model(seed)
    _, q, hidden = R.act(model, inputs, hidden=True)
    assert len(np.unique(q)) > 50, len(np.unique(q))
    for k, h in enumerate(hidden):
        assert len(np.unique(h)) > 50, (k, len(np.unique(h)))
        assert h.min() == model["layers"][k]["oz"], "ReLU clamps at the code of real 0"
    assert model["input_zero"] != 0 and model["action_zero"] != 0 and all(L["oz"] != 0 for L in model["layers"])
    for L in model["layers"][:2]:
        ts = [R.multiplier(float(bs) / L["os"])[1] for bs in L["bs"][2:4]]
        assert ts == [62, 1], "one channel at each end of the valid shifts"


def test_edge_unit_models_read_one_unit(inputs):
    """the action code of an edge model is a function of ONE hidden code: perturbing any other unit's row changes nothing, and
    perturbing the unit's own row changes the output; more than 8 distinct codes each (the base is random_model(4): see
    tests/qactor_arch_cases.py)"""
    assert A.EDGE_UNITS == ((0, 31, 32, 223, 224, 255),) * 2
    for layer, units in enumerate(A.EDGE_UNITS):
        for unit in units:
            model = A.edge_unit_model(layer, unit)
            q = R.act(model, inputs[:512])[1]
            other = (unit + 1) % model["layers"][layer]["W"].shape[0]
            for row, changes in ((other, False), (unit, True)):
                m2 = A.edge_unit_model(layer, unit)
                m2["layers"][layer]["W"][row] = -m2["layers"][layer]["W"][row]
                m2["layers"][layer]["b"][row] = -m2["layers"][layer]["b"][row]
                assert (not np.array_equal(R.act(m2, inputs[:512])[1], q)) == changes, (layer, unit, row)
            assert len(np.unique(q)) > 8, (layer, unit, len(np.unique(q)))


def test_special_values_follow_the_specification():
    """NaN -> the zero point, +-Inf and +-1e30 saturate: a row of NaN is a row of zero observations"""
    model = K.random_model(0)
    a, q = R.act(model, K.special_rows()[:5])
    a0, q0 = R.act(model, np.zeros((1, 6), np.float32))
    assert np.array_equal(q[0], q0[0]) and np.array_equal(q[1], q[3]) and np.array_equal(q[2], q[4])
    assert not np.array_equal(q[1], q[2])


def test_weights_of_minus_128_are_allowed(host):
    model = K.random_model(0)
    model["layers"][1]["W"][:, ::3] = -128
    obs = K.seeded_obs(65)
    assert np.array_equal(host_act(host, model, obs)[1], R.act(model, obs)[1])


# ------------------------------------------------------------------------------------- 2. the sanitised stand-alone program
def _fnv(data):
    h = 14695981039346656037
    for b in data:
        h = ((h ^ b) * 1099511628211) & (2 ** 64 - 1)
    return h


def test_standalone_program_is_clean_under_asan_and_ubsan(models, inputs, tmp_path):
    """qactorarchhost_main.cpp has its own main: nothing sanitized is loaded into Python.  Both builds exit 0 and print the same
    digests, and they are the digests of the reference's outputs.  The cases: a random model, the shift ends on the output, the
    last unit of the last tile of each hidden layer, the PD actor"""
    paths, want = [], ""
    rows = np.ascontiguousarray(np.concatenate([inputs[-15:], inputs[:242]]), np.float32)
    picked = (models[0], models[3], models[9], models[15], models[16])
    assert [name for name, _ in picked][2:4] == ["edge/layer0/unit255", "edge/layer1/unit255"]
    for name, model in picked:
        path = tmp_path / (name.replace("/", "_") + ".bin")
        with open(path, "wb") as f:
            f.write(np.array([rows.shape[0]], np.int32).tobytes())
            f.write(np.array([model["input_scale"], model["action_scale"]], np.float64).tobytes())
            f.write(np.array([model["input_zero"], model["action_zero"]], np.int32).tobytes())
            for L in model["layers"]:
                f.write(np.array([L["os"]], np.float64).tobytes() + np.array([L["oz"]], np.int32).tobytes())
                f.write(np.ascontiguousarray(L["W"], np.int8).tobytes() + np.ascontiguousarray(L["b"], np.int32).tobytes())
                f.write(np.ascontiguousarray(L["bs"], np.float64).tobytes())
            f.write(R.tanh_table(model).astype(np.int8).tobytes() + rows.tobytes())
        paths.append(str(path))
        a, q = R.act(model, rows)
        want += f"n={rows.shape[0]} action={_fnv(a.tobytes()):016x} codes={_fnv(q.tobytes()):016x}\n"
    out = {}
    for name, flags in (("plain", []), ("san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / f"qactorarchhost_{name}")
        subprocess.check_call(GXX + flags + ["-o", exe, os.path.join(HOST_DIR, "qactorarchhost_main.cpp")])
        r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        out[name] = r.stdout
    assert out["plain"] == out["san"] == want


# ------------------------------------------------------------------------------------------- 3. the quantiser, net_arch="sb3"
def _tiny_actor():
    """tests/test_qactor_cpu.py's hand-computed actor at [256, 256], DDPG layout: a few non-zero weights, and two of them moved to
    the last unit of each hidden layer (255), which the reference widths do not have"""
    W0, b0 = np.zeros((256, 6)), np.zeros(256)
    W0[0, 0], b0[0] = 1.0, 0.5
    W0[255, :3] = (-0.5, 0.25, -0.25)
    b0[2] = -1.0                                   # an all-zero row under a negative bias
    W1, b1 = np.zeros((256, 256)), np.zeros(256)
    W1[0, 0] = 2.0
    W1[255, 255], b1[255] = 1.0, 0.2
    W2, b2 = np.zeros((2, 256)), np.zeros(2)
    W2[0, 0], b2[0] = 0.1, -0.1
    W2[1, 255] = -0.5
    return np.concatenate([W0.ravel(), b0, W1.ravel(), b1, W2.ravel(), b2])


TINY_CAL = np.array([[-2.0] * 6, [0.0] * 6, [2.0] * 6])


def test_quantiser_known_answers():
    """calibration rows -2, 0, 2 on every input.  Input: scale 4/255, zero point round(-128 + 127.5) = round(-0.5) = -1 (half
    away).  Layer 0: unit 0 = x + 0.5 -> post-ReLU (0, 0.5, 2.5); unit 255 = -0.5x + 0.25x - 0.25x -> (1, 0, 0); unit 2 = -1 -> 0:
    range [0, 2.5].  Layer 1: unit 0 = 2 h0 -> (0, 1, 5); unit 255 = h255 + 0.2 -> (1.2, 0.2, 0.2): range [0, 5].  Layer 2: unit 0
    = 0.1 (0, 1, 5) - 0.1 = (-0.1, 0, 0.4); unit 1 = -0.5 (1.2, 0.2, 0.2) = (-0.6, -0.1, -0.1): range [-0.6, 0.4], scale 1/255,
    zero point round(-128 + 153) = 25.  The numbers are those of the reference widths' test: the rules do not know the widths"""
    qm = A.quantize(_tiny_actor(), TINY_CAL)
    assert qm.net_arch == "sb3" and [L["W"].shape for L in qm.layers] == [(256, 6), (256, 256), (2, 256)]
    near = lambda a, b: abs(a / b - 1) < 1e-12
    assert near(qm.input_scale, 4 / 255) and qm.input_zero == -1
    L0, L1, L2 = qm.layers
    assert [L["W"].dtype for L in qm.layers] == [np.int8] * 3 and [L["b"].dtype for L in qm.layers] == [np.int32] * 3
    # layer 0
    assert near(L0["ws"][0], 1 / 127) and near(L0["ws"][255], 0.5 / 127) and L0["ws"][2] == 1.0, "an all-zero row has weight scale 1"
    assert list(L0["W"][0]) == [127, 0, 0, 0, 0, 0] and list(L0["W"][255]) == [-127, 64, -64, 0, 0, 0], "63.5 rounds away from zero"
    assert not L0["W"][1:255].any()
    assert near(L0["bs"][0], 4 / 255 / 127) and L0["b"][0] == 4048 and L0["b"][255] == 0     # 0.5 x 127 x 255 / 4 = 4048.125
    assert L0["b"][2] == -64 and near(L0["bs"][2], 4 / 255)                                 # -1 / (4 / 255) = -63.75
    assert near(L0["os"], 2.5 / 255) and L0["oz"] == -128
    # layer 1: its input scale is layer 0's output scale
    assert near(L1["ws"][0], 2 / 127) and L1["W"][0, 0] == 127 and L1["W"][255, 255] == 127 and int(np.abs(L1["W"]).sum()) == 254
    assert near(L1["bs"][255], 2.5 / 255 / 127) and L1["b"][255] == 2591                    # 0.2 x 127 x 255 / 2.5 = 2590.8
    assert near(L1["os"], 5 / 255) and L1["oz"] == -128
    # layer 2: an asymmetric range
    assert L2["W"][0, 0] == 127 and L2["W"][1, 255] == -127 and int(np.abs(L2["W"]).sum()) == 254
    assert near(L2["bs"][0], 5 / 255 * 0.1 / 127) and L2["b"][0] == -6477 and L2["b"][1] == 0   # -0.1 x 127 x 255 / 0.5
    assert near(L2["os"], 1 / 255) and L2["oz"] == 25
    # the table: tanh((q - 25) / 255) x 128, half to even
    assert qm.action_scale == 1 / 128 and qm.action_zero == 0
    t = qm.table()
    assert t.dtype == np.int8 and t.shape == (256,)
    assert t[25 + 128] == 0 and t[127 + 128] == 49 and t[0] == -69      # tanh(0.4) x 128 = 48.63, tanh(-0.6) x 128 = -68.74
    assert [int(v) for v in t] == [int(np.rint(math.tanh((q - 25) / 255) * 128)) for q in range(-128, 128)]
    assert np.array_equal(t.astype(np.int64), R.tanh_table(K.as_ref_model(qm)))


def _arrays_equal(a, b):
    a, b = a.arrays(), b.arrays()
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)


def test_quantiser_reads_every_form_of_a_256_wide_sac_actor():
    """the flat vector with and without log_ent_coef and both state_dict namings give equal models; the log_std head and
    log_ent_coef change nothing; the layers are those of the DDPG-layout vector the mu head is"""
    flat = K.sb3_init_params(3)
    rng = np.random.default_rng(0)
    sac = lambda: A.sac_vector(flat, rng.normal(0, 1, (2, 256)), rng.normal(0, 1, 2), rng.normal())
    a, b = sac(), sac()
    assert not np.array_equal(a, b) and a.size == _lib.SAC256_NACTOR + 1 == 68613
    want = quantize_actor(A.sac_vector(flat), head="sac", net_arch="sb3")
    for v in (a, b, a[:-1], unflatten_sac_actor(a, "sb3"), unflatten_sac_actor(b, "tool")):
        assert _arrays_equal(quantize_actor(v, head="sac", net_arch="sb3"), want), "the mu head is quantised; log_std changes nothing"
    # the same rules as at the reference widths: every non-zero row uses +-127, each weight within half a step of its code
    off = 0
    for L, (n_in, n_out) in zip(want.layers, A.SIZES):
        W = flat[off:off + n_in * n_out].astype(np.float64).reshape(n_out, n_in); off += n_in * n_out + n_out
        assert (np.abs(L["W"].astype(int)).max(axis=1) == 127).all()
        assert (np.abs(W - L["ws"][:, None] * L["W"]) <= L["ws"][:, None] / 2 * (1 + 1e-12)).all()
    assert [L["oz"] for L in want.layers[:2]] == [-128, -128]


def test_quantiser_errors():
    from tests import qactor_cases as K0
    sac256 = A.sac_vector(K.sb3_init_params(1))
    n01 = K0.NACTOR - 402
    f0 = K0.sb3_init_params(1)
    sac_ref = np.concatenate([f0[:n01 + 400], np.zeros(400, np.float32), f0[n01 + 400:], np.zeros(3, np.float32)])
    assert sac_ref.size == _lib.SAC_NACTOR + 1
    quantize_actor(sac_ref, head="sac")                                    # the default serves the reference widths as before
    # the default net_arch still refuses a [256, 256] actor, and now says what to pass
    for v in (sac256, sac256[:-1], unflatten_sac_actor(sac256, "sb3")):
        with pytest.raises(ValueError, match=r"\[256, 256\] SAC actor .* reference widths pi=\[300, 200\].*net_arch='sb3'"):
            quantize_actor(v, head="sac")
    with pytest.raises(ValueError, match="head='sac'"):
        quantize_actor(sac256, head="ddpg", net_arch="sb3")
    with pytest.raises(ValueError, match="head='sac'"):
        quantize_actor(sac256, net_arch="sb3")
    for v in (sac_ref, sac_ref[:-1], unflatten_sac_actor(sac_ref, "tool")):
        with pytest.raises(ValueError, match="net_arch='reference'"):
            quantize_actor(v, head="sac", net_arch="sb3")                  # a reference-width vector
    with pytest.raises(ValueError, match="68612"):
        quantize_actor(f0, head="sac", net_arch="sb3")                     # a DDPG vector is no SAC vector
    with pytest.raises(ValueError, match="68612"):
        quantize_actor(K.sb3_init_params(1), head="sac", net_arch="sb3")   # nor is the DDPG layout at these widths
    with pytest.raises(ValueError, match="net_arch must be"):
        quantize_actor(sac256, head="sac", net_arch="td3")
    with pytest.raises(ValueError, match="head must be"):
        quantize_actor(sac256, head="ppo", net_arch="sb3")
    for bad in (np.nan, np.inf):
        p = sac256.copy()
        p[1234] = bad
        with pytest.raises(ValueError, match="not finite"):
            quantize_actor(p, head="sac", net_arch="sb3")
        cal = TINY_CAL.copy()
        cal[1, 2] = bad
        with pytest.raises(ValueError, match="calibration_obs"):
            quantize_actor(sac256, cal, head="sac", net_arch="sb3")
    # a non-finite log_std head is not the quantiser's business: it is dropped
    p = sac256.copy()
    p[A.NACTOR] = np.nan
    assert _arrays_equal(quantize_actor(p, head="sac", net_arch="sb3"), quantize_actor(sac256, head="sac", net_arch="sb3"))
    zero = quantize_actor(np.zeros(_lib.SAC256_NACTOR, np.float32), np.zeros((2, 6)), head="sac", net_arch="sb3")
    assert [(L["os"], L["oz"]) for L in zero.layers] == [(1.0, -128), (1.0, -128), (1.0, 0)], "a degenerate range gets scale 1"


def test_model_reads_its_widths_off_the_tensors():
    from tests import qactor_cases as K0
    m256, m300 = K.quant_model(K.random_model(0)), K0.quant_model(K0.random_model(0))
    assert (m256.net_arch, m300.net_arch) == ("sb3", "reference")
    assert m256.float_params().shape == (68098,) and m300.float_params().shape == (62702,)
    cm, keep = m256.c_model()
    assert [(cm.layer[k].n_in, cm.layer[k].n_out) for k in range(3)] == [(6, 256), (256, 256), (256, 2)]
    layers = lambda m: [dict(L) for L in m.layers]
    args = lambda m: (m.input_scale, m.input_zero)
    bad = layers(m256); bad[0]["W"] = np.zeros((128, 6), np.int8)
    with pytest.raises(ValueError, match=r"layer 0: .*\(300, 6\).*\(256, 6\)"):
        QuantActorModel(*args(m256), bad)
    mixed = layers(m256); mixed[1] = layers(m300)[1]
    with pytest.raises(ValueError, match=r"layer 1: .*\(256, 256\).*\(200, 300\)"):
        QuantActorModel(*args(m256), mixed)
    mixed = layers(m300); mixed[2] = layers(m256)[2]
    with pytest.raises(ValueError, match=r"layer 2: .*\(2, 200\).*\(2, 256\)"):
        QuantActorModel(*args(m300), mixed)


# ---------------------------------------------------------------------------------------------------- 4. quantiser quality
@pytest.fixture(scope="module")
def quality_cases():
    return {"pd": A.pd_actor_params(), "sb3": K.sb3_init_params()}


@pytest.mark.parametrize("which", ["pd", "sb3"])
def test_quantised_actor_is_close_to_the_float_actor(quality_cases, which):
    """a measurement of the QUANTISER against the fp64 float network on 4,096 observations inside the calibration box, not of the
    kernel.  Measured max |delta action| at [256, 256]: pd 0.25027, sb3 0.09989; the gate is twice that"""
    flat, obs = quality_cases[which], K.in_box_obs(4096)
    a = R.act(K.as_ref_model(A.quantize(flat)), obs)[0]
    err = float(np.abs(a.astype(np.float64) - A.float_actor(flat, obs)).max())
    print(f"{which}: max |delta action| {err:.5f} (measured {MEASURED_MAX_ERR[which]})")
    assert err <= 2 * MEASURED_MAX_ERR[which]


def test_pd_actor_embeds_the_linear_law():
    """relu(f) - relu(-f) = f through both hidden layers, transplanted to these widths: without the seeded small weights the float
    actor IS tanh(law); with them it stays within 0.02 of it (256 weights of sd 0.002 on activations of order 1)"""
    obs = K.in_box_obs(512)
    flat = A.pd_actor_params().astype(np.float64)
    pure = flat.copy()
    n01 = A.NACTOR - 2 * 256 - 2
    W2 = pure[n01:n01 + 2 * 256].reshape(2, 256)
    W2[:, 4:] = 0.0
    np.testing.assert_allclose(A.float_actor(pure, obs), np.tanh(K.pd_law(obs)), rtol=0, atol=1e-6)   # float32 parameters
    assert np.abs(A.float_actor(flat, obs) - np.tanh(K.pd_law(obs))).max() < 0.02


# ------------------------------------------------------------------------------------------------------ 5. file round trip
def test_file_round_trip(quality_cases, tmp_path):
    qm = A.quantize(quality_cases["pd"])
    path = str(tmp_path / "pd_actor256.npz")
    qm.save(path)
    z = np.load(path, allow_pickle=False)
    keys = ["input_scale", "input_zero_point", "action_scale", "action_zero_point"] + \
           [f"fc{k}_{s}" for k in range(3) for s in ("weight_q", "weight_scale", "bias_q", "bias_scale", "out_scale", "out_zero_point")]
    assert sorted(z.files) == sorted(keys), "the key set of the reference widths' file"
    back = QuantActorModel.load(path)
    assert back.net_arch == "sb3" and _arrays_equal(qm, back)
    obs = K.seeded_obs(1025)
    a, q = R.act(K.as_ref_model(qm), obs)
    a2, q2 = R.act(K.as_ref_model(back), obs)
    assert np.array_equal(a, a2) and np.array_equal(q, q2)
    assert np.array_equal(back.table(), qm.table())
    # the dequantised float network stays within the quantiser's bound of the float actor
    fp = back.float_params()
    assert fp.dtype == np.float32 and fp.shape == (A.NACTOR,)
    box = K.in_box_obs(4096)
    err = float(np.abs(A.float_actor(fp, box) - A.float_actor(quality_cases["pd"], box)).max())
    print(f"float_params vs the float actor: {err:.5f}")
    assert err <= 2 * MEASURED_MAX_ERR["pd"]


def test_train_tool_actor_files_are_read_back(tmp_path):
    """what tools/train_sac_torch.py --net-arch sb3 --save-actor writes -- np.save of the actor vector [SAC256_NACTOR + 1], or
    torch.save of unflatten_sac_actor(vector, "tool") -- read the way tools/eval_quant_policy.py --actor reads it"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eval_quant_policy as E
    vec = A.sac_vector(K.sb3_init_params(2), log_ent_coef=-1.5)
    want = quantize_actor(vec, head="sac", net_arch="sb3")
    np.save(str(tmp_path / "actor.npy"), vec)
    torch.save(unflatten_sac_actor(vec, "tool"), str(tmp_path / "actor.pt"))
    for name in ("actor.npy", "actor.pt"):
        params, flat, net_arch = E.read_sac_actor(str(tmp_path / name))
        assert net_arch == "sb3" and flat.shape == (_lib.SAC256_NACTOR + 1,) and np.array_equal(flat, vec)
        assert _arrays_equal(quantize_actor(params, head="sac", net_arch=net_arch), want)
    from tests import qactor_cases as K0
    f0, n01 = K0.sb3_init_params(1), K0.NACTOR - 402
    np.save(str(tmp_path / "actor_ref.npy"), np.concatenate([f0[:n01 + 400], np.zeros(400, np.float32), f0[n01 + 400:], np.zeros(2, np.float32)]))
    _, flat, net_arch = E.read_sac_actor(str(tmp_path / "actor_ref.npy"))
    assert net_arch == "reference" and flat.shape == (_lib.SAC_NACTOR + 1,), "log_ent_coef is appended when the file has none"
    np.save(str(tmp_path / "short.npy"), np.zeros(100, np.float32))
    with pytest.raises(ValueError, match="68612"):
        E.read_sac_actor(str(tmp_path / "short.npy"))


# ------------------------------------------------- 6. the library's checks at these widths, without a device: check_model
def _check(arch, model, mutate=None):
    cm, keep = K.c_model(model)
    if mutate:
        keep.append(mutate(cm))
    L = _lib.lib()
    rc = L.brs_qpolicy_actor_check_model(arch, C.byref(cm))
    return rc, L.brs_qpolicy_actor_last_error(None).decode()


def test_check_model_applies_every_rule_at_the_new_widths():
    """every rule of tests/test_qactor_cpu.py::test_set_model_checks_the_model_before_the_handle, violated once on a 6-256-256-2
    model, with the exact message"""
    def sizes(cm): cm.layer[1].n_in = 320
    def sizes_out(cm): cm.layer[2].n_out = 1
    def table_on_hidden(cm): cm.layer[1].tanh_table = cm.layer[2].tanh_table
    def no_table_on_output(cm): cm.layer[2].tanh_table = None
    def zero_point(cm): cm.layer[1].out_zero = 200
    def input_zero(cm): cm.input_zero = -129
    def action_zero(cm): cm.action_zero = 128
    def input_scale(cm): cm.input_scale = 0.0
    def action_scale(cm): cm.action_scale = math.inf
    def out_scale(cm): cm.layer[0].out_scale = -1.0
    def bias_scale(cm):
        bs = np.full(256, 1e-3); bs[255] = math.nan
        cm.layer[1].bias_scale = bs.ctypes.data
        return bs
    def multiplier(cm): cm.layer[0].out_scale = 1e-30
    def bias(cm):
        b = np.zeros(256, np.int32); b[255] = 2 ** 31 - 1 - 1000   # + 256 x 127 x 128 leaves int32
        cm.layer[1].bias = b.ctypes.data
        return b
    def null_weights(cm): cm.layer[0].weight = None
    model = K.random_model(0)
    assert _check(1, model)[0] == OK, "a good model"
    for mutate, text in ((sizes, "layer 1: the network must be 6-256-256-2"), (sizes_out, "layer 2: the network must be 6-256-256-2"),
                         (table_on_hidden, "layer 1: a hidden layer takes no table"), (no_table_on_output, "layer 2: the output layer needs a tanh table"),
                         (zero_point, "layer 1: out_zero outside [-128, 127]"), (input_zero, "input_zero outside [-128, 127]"),
                         (action_zero, "action_zero outside [-128, 127]"), (input_scale, "input_scale must be positive and finite"),
                         (action_scale, "action_scale must be positive and finite"), (out_scale, "layer 0: out_scale must be positive and finite"),
                         (bias_scale, "layer 1, channel 255: bias_scale must be positive and finite"),
                         (multiplier, "layer 0, channel 0: bias_scale / out_scale is not a valid multiplier"),
                         (bias, "layer 1, channel 255: the accumulator can leave int32"), (null_weights, "layer 0: null pointer")):
        rc, msg = _check(1, model, mutate)
        assert rc == ERR_ARG and msg == "brs_qpolicy_actor_set_model: " + text, (mutate.__name__, rc, msg)
    L = _lib.lib()
    assert L.brs_qpolicy_actor_check_model(1, None) == ERR_ARG
    assert L.brs_qpolicy_actor_last_error(None).decode() == "brs_qpolicy_actor_set_model: null argument"


def test_the_accumulator_bound_uses_k_256():
    """layer 1 reads K = 256 codes.  With the quantiser's zero point oz0 = -128 the largest |q - oz0| is 255, and a channel of
    all-127 weights has sum |W| = 256 x 127.  As specified, |b| + 256 x 127 x 255 must fit int32; as computed, the folded bias is
    b + 128 x 256 x 127 and |folded| + 256 x 127 x 128 must.  For b > 0 the second is the tighter (256 x 127 x 256 in all), for
    b < 0 the first: both limits are exact, one more is refused"""
    model = K.random_model(0)
    model["layers"][0]["oz"] = -128
    model["layers"][1]["W"][7] = 127
    i32 = 2 ** 31 - 1
    pos, neg = i32 - 256 * 127 * 256, i32 - 256 * 127 * 255
    assert pos > i32 - 300 * 127 * 255, "a bound computed for K = 300 would refuse a bias that K = 256 allows"
    for b, ok in ((pos, True), (pos + 1, False), (-neg, True), (-neg - 1, False)):
        model["layers"][1]["b"][7] = b
        rc, msg = _check(1, model)
        assert rc == (OK if ok else ERR_ARG), (b, rc, msg)
        assert ok or msg == "brs_qpolicy_actor_set_model: layer 1, channel 7: the accumulator can leave int32"


def test_check_model_dispatches_on_the_architecture():
    from tests import qactor_cases as K0
    m256, m300 = K.random_model(0), K0.random_model(0)
    assert _check(0, m300)[0] == OK and _check(1, m256)[0] == OK
    assert _check(0, m256) == (ERR_ARG, "brs_qpolicy_actor_set_model: layer 0: the network must be 6-300-200-2")
    assert _check(1, m300) == (ERR_ARG, "brs_qpolicy_actor_set_model: layer 0: the network must be 6-256-256-2")
    def zero_point(cm): cm.layer[1].out_zero = 200
    assert _check(0, m300, zero_point) == (ERR_ARG, "brs_qpolicy_actor_set_model: layer 1: out_zero outside [-128, 127]")
    for arch in (7, -1, 2):
        rc, msg = _check(arch, m256)
        assert rc == ERR_ARG and msg.startswith(f"brs_qpolicy_actor_check_model: unknown architecture {arch}"), (arch, msg)


def test_set_model_without_a_handle_is_the_reference_widths():
    L = _lib.lib()
    cm, keep = K.c_model(K.random_model(0))
    assert L.brs_qpolicy_actor_set_model(None, C.byref(cm)) == ERR_ARG
    assert L.brs_qpolicy_actor_last_error(None).decode() == "brs_qpolicy_actor_set_model: layer 0: the network must be 6-300-200-2"


def test_create_arch_checks_its_arguments():
    L = _lib.lib()
    h = C.c_void_p()
    assert L.brs_qpolicy_actor_create_arch(0, 7, C.byref(h)) == ERR_ARG and h.value is None
    assert L.brs_qpolicy_actor_last_error(None).decode().startswith("brs_qpolicy_actor_create_arch: unknown architecture 7")
    assert L.brs_qpolicy_actor_create_arch(0, 1, None) == ERR_ARG
    assert L.brs_qpolicy_actor_last_error(None).decode() == "brs_qpolicy_actor_create_arch: null argument"
    assert L.brs_qpolicy_actor_create_arch(0, 0, None) == ERR_ARG
    assert L.brs_qpolicy_actor_last_error(None).decode() == "brs_qpolicy_actor_create: null argument", "arch 0 is brs_qpolicy_actor_create"


def test_symbols_are_exported_and_in_the_table():
    L = _lib.lib()
    names = ["brs_qpolicy_actor_create_arch", "brs_qpolicy_actor_check_model"]
    assert all(hasattr(L, s) and s in _lib.SIGNATURES["brs_qpolicy.h"] and s in _lib.QPOLICY_SYMBOLS for s in names)
    header = open(os.path.join(ROOT, "include", "brs_qpolicy.h")).read()
    for text in ("#define BRS_QACTOR256_H0 256", "#define BRS_QACTOR256_H1 256", "#define BRS_QACTOR_ARCH_REFERENCE 0",
                 "#define BRS_QACTOR_ARCH_SAC_DEFAULT 1", "int brs_qpolicy_actor_create_arch(int32_t device, int32_t arch, brs_qactor** out);",
                 "int brs_qpolicy_actor_check_model(int32_t arch, const brs_qactor_model*);"):
        assert text in header, text
    assert (_lib.ARCH_REFERENCE, _lib.ARCH_SAC_DEFAULT) == (0, 1)
