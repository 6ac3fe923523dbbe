"""The flat parameter vectors of the off-policy networks, pinned to the commit before the Python layer got its one network table
(tests/golden/flat_vectors_parent.json): the six flatten / unflatten functions of offpolicy.py and quant._actor_flat, for both
namings and both width sets, on seeded state_dicts.  The fixture holds the SHA-256 of every flat vector and of every unflattened
tensor, and the text of the error every single-fault input raises: a tensor missing, a tensor with one dimension changed, widths of
two architectures in one dict, a flat vector of the wrong length.  The names and shapes below are written out by hand on purpose:
nothing here is derived from the tables under test.

BRS_WRITE_FLAT_VECTORS=1 writes the fixture from what the code under test returns; it was run once, on that parent commit."""
import functools
import hashlib
import json
import os

import numpy as np

from balance_robot_mujoco_rl_amd import offpolicy, quant

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flat_vectors_parent.json")
PI, QF = {"reference": (300, 200), "sb3": (256, 256)}, {"reference": (200, 150), "sb3": (256, 256)}
DDPG_PREFIX = {"sb3": {"actor": "actor.mu.{}.", "critic": "critic.qf0.{}.", "actor_target": "actor_target.mu.{}.", "critic_target": "critic_target.qf0.{}."},
               "tool": {"actor": "actor.{}.", "critic": "critic.{}.", "actor_target": "actor_target.{}.", "critic_target": "critic_target.{}."}}
TD3_PREFIX = {"sb3": "{net}.qf{k}.{i}.", "tool": "{net}.{k}.{i}."}
SAC_BODY = {"sb3": "actor.latent_pi.{}.", "tool": "actor.body.{}."}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _linear(rng, sd, prefix, n_out, n_in):
    sd[prefix + "weight"], sd[prefix + "bias"] = rng.uniform(-1.0, 1.0, (n_out, n_in)), rng.uniform(-1.0, 1.0, (n_out,))


def ddpg_sd(net, naming):
    rng, sd = np.random.default_rng(0), {}
    n_in, (h0, h1), n_out = (6, PI["reference"], 2) if net.startswith("actor") else (8, QF["reference"], 1)
    for i, (o, n) in zip((0, 2, 4), ((h0, n_in), (h1, h0), (n_out, h1))):
        _linear(rng, sd, DDPG_PREFIX[naming][net].format(i), o, n)
    return sd


def td3_sd(net, naming, widths):
    rng, sd = np.random.default_rng(0), {}
    h0, h1 = QF[widths]
    for k in (0, 1):
        for i, (o, n) in zip((0, 2, 4), ((h0, 8), (h1, h0), (1, h1))):
            _linear(rng, sd, TD3_PREFIX[naming].format(net=net, k=k, i=i), o, n)
    return sd


def sac_sd(naming, widths):
    """in SB3's key order, which is not the flat order: mu's weight and bias, then log_std's"""
    rng, sd = np.random.default_rng(0), {}
    h0, h1 = PI[widths]
    _linear(rng, sd, SAC_BODY[naming].format(0), h0, 6); _linear(rng, sd, SAC_BODY[naming].format(2), h1, h0)
    _linear(rng, sd, "actor.mu.", 2, h1); _linear(rng, sd, "actor.log_std.", 2, h1)
    sd["log_ent_coef"] = rng.uniform(-1.0, 1.0, (1,))
    return sd


def _outcome(f):
    """what a call gives: the hash of a flat vector, the hashes of a dict's tensors in key order, or the error's text"""
    try:
        r = f()
    except Exception as e:   # the text is what is pinned, whatever the type
        return {"error": f"{type(e).__name__}: {e}"}
    if isinstance(r, dict):
        return {"tensors": [[k, list(v.shape), str(v.numpy().dtype), _sha(v.numpy())] for k, v in r.items()]}
    return {"flat": [list(r.shape), str(r.dtype), _sha(r)]}


def _faults(sd):
    """(label, dict) for every single fault: each tensor missing, each tensor with its last dimension one longer"""
    for name in sd:
        yield f"missing {name}", {k: v for k, v in sd.items() if k != name}
        a = sd[name]
        yield f"reshaped {name}", {**sd, name: np.zeros(a.shape[:-1] + (a.shape[-1] + 1,))}


def _function_pair(out, key, sd, flatten, unflatten):
    flat = flatten(sd)
    out[f"{key} flatten"] = _outcome(lambda: flat)
    out[f"{key} unflatten"] = _outcome(lambda: unflatten(flat))
    assert flatten(unflatten(flat)).tobytes() == flat.tobytes(), key
    assert flatten({k: v.astype(np.float32) for k, v in sd.items()}).tobytes() == flat.tobytes(), key   # the cast is the function's


@functools.lru_cache(maxsize=None)
def observed():
    out, O = {}, offpolicy
    # ---- DDPG: four networks, two namings, the reference widths
    for naming in ("sb3", "tool"):
        for net in ("actor", "critic", "actor_target", "critic_target"):
            sd, key = ddpg_sd(net, naming), f"ddpg {net} {naming}"
            _function_pair(out, key, sd, lambda s: O.flatten_ddpg_state_dict(s, net), lambda f: O.unflatten_ddpg_state_dict(f, net, naming))
            if net in ("actor", "critic"):
                for label, bad in _faults(sd):
                    out[f"{key} {label}"] = _outcome(lambda: O.flatten_ddpg_state_dict(bad, net))
                n = O.flatten_ddpg_state_dict(sd, net).size
                out[f"{key} wrong length"] = _outcome(lambda: O.unflatten_ddpg_state_dict(np.zeros(n + 1, np.float32), net, naming))
    out["ddpg no naming"] = _outcome(lambda: O.flatten_ddpg_state_dict({}, "actor"))
    # ---- TD3 / SAC critics: two networks, two namings, two width sets
    for naming in ("sb3", "tool"):
        for widths in ("reference", "sb3"):
            for net in ("critic", "critic_target"):
                sd, key = td3_sd(net, naming, widths), f"td3 {net} {naming} {widths}"
                _function_pair(out, key, sd, lambda s: O.flatten_td3_critics(s, net), lambda f: O.unflatten_td3_critics(f, net, naming))
            sd, key = td3_sd("critic", naming, widths), f"td3 critic {naming} {widths}"
            for label, bad in _faults(sd):
                out[f"{key} {label}"] = _outcome(lambda: O.flatten_td3_critics(bad, "critic"))
            n = O.flatten_td3_critics(sd, "critic").size
            out[f"{key} wrong length"] = _outcome(lambda: O.unflatten_td3_critics(np.zeros(n + 1, np.float32), "critic", naming))
        last = TD3_PREFIX[naming].format(net="critic", k=1, i=4) + "weight"
        out[f"td3 critic {naming} mixed widths"] = _outcome(lambda: O.flatten_td3_critics({**td3_sd("critic", naming, "sb3"), last: np.zeros((1, 150))}, "critic"))
    out["td3 no naming"] = _outcome(lambda: O.flatten_td3_critics({}, "critic"))
    out["td3 bad net"] = _outcome(lambda: O.unflatten_td3_critics(np.zeros(64202, np.float32), "actor", "sb3"))
    out["td3 bad naming"] = _outcome(lambda: O.unflatten_td3_critics(np.zeros(64202, np.float32), "critic", "sb4"))
    # ---- the SAC actor: two namings, two width sets
    for naming in ("sb3", "tool"):
        for widths in ("reference", "sb3"):
            sd, key = sac_sd(naming, widths), f"sac {naming} {widths}"
            _function_pair(out, key, sd, O.flatten_sac_actor, lambda f: O.unflatten_sac_actor(f, naming))
            for label, bad in _faults(sd):
                out[f"{key} {label}"] = _outcome(lambda: O.flatten_sac_actor(bad))
            flat = O.flatten_sac_actor(sd)
            for shape in ((), (1, 1)):   # log_ent_coef: any tensor of one element
                assert O.flatten_sac_actor({**sd, "log_ent_coef": sd["log_ent_coef"].reshape(shape)}).tobytes() == flat.tobytes()
            out[f"{key} wrong length"] = _outcome(lambda: O.unflatten_sac_actor(np.zeros(flat.size + 1, np.float32), naming))
        # the dict of tests/test_sac_arch_cpu.py: every tensor fits one of the two architectures, not the same one
        out[f"sac {naming} mixed widths"] = _outcome(lambda: O.flatten_sac_actor({**sac_sd(naming, "sb3"), "actor.mu.weight": np.zeros((2, 200))}))
    out["sac no naming"] = _outcome(lambda: O.flatten_sac_actor({"log_ent_coef": np.zeros(1)}))
    out["sac bad naming"] = _outcome(lambda: O.unflatten_sac_actor(np.zeros(63105, np.float32), "sb4"))
    # ---- quant._actor_flat: the fp64 DDPG-layout vector, from a state_dict and from the flat vector, with and without log_ent_coef
    ddpg = ddpg_sd("actor", "sb3")
    sac = {w: sac_sd("sb3", w) for w in ("reference", "sb3")}
    sac_flat = {w: O.flatten_sac_actor(sd) for w, sd in sac.items()}
    for net_arch in ("reference", "sb3"):
        out[f"quant ddpg {net_arch} dict"] = _outcome(lambda: quant._actor_flat(ddpg, "ddpg", net_arch))
        out[f"quant ddpg {net_arch} flat"] = _outcome(lambda: quant._actor_flat(O.flatten_ddpg_state_dict(ddpg), "ddpg", net_arch))
        for given in ("reference", "sb3"):   # given == net_arch: served; the other: refused by name
            key = f"quant sac {net_arch} given {given}"
            out[f"{key} dict"] = _outcome(lambda: quant._actor_flat(sac[given], "sac", net_arch))
            out[f"{key} flat"] = _outcome(lambda: quant._actor_flat(sac_flat[given], "sac", net_arch))
            out[f"{key} flat without log_ent_coef"] = _outcome(lambda: quant._actor_flat(sac_flat[given][:-1], "sac", net_arch))
        out[f"quant sac {net_arch} wrong length"] = _outcome(lambda: quant._actor_flat(np.zeros(1000), "sac", net_arch))
    out["quant ddpg wrong length"] = _outcome(lambda: quant._actor_flat(np.zeros(1000), "ddpg", "reference"))
    out["quant bad head"] = _outcome(lambda: quant._actor_flat(ddpg, "td3", "reference"))
    out["quant bad net_arch"] = _outcome(lambda: quant._actor_flat(ddpg, "ddpg", "td3"))
    return out


def _golden():
    if os.environ.get("BRS_WRITE_FLAT_VECTORS") == "1":
        with open(GOLDEN, "w") as f:
            json.dump(observed(), f, indent=0, sort_keys=True)
            f.write("\n")
    with open(GOLDEN) as f:
        return json.load(f)


def _compare(prefix):
    want, got = _golden(), observed()
    assert sorted(k for k in want if k.startswith(prefix)) == sorted(k for k in got if k.startswith(prefix))
    keys = [k for k in want if k.startswith(prefix)]
    assert keys
    for k in keys:
        assert got[k] == want[k], k
    return {k: want[k] for k in keys}


def test_ddpg_vectors_tensors_and_errors_are_the_parents():
    w = _compare("ddpg ")
    assert w["ddpg actor sb3 flatten"]["flat"][:2] == [[62702], "float32"] and w["ddpg critic tool flatten"]["flat"][0] == [32101]
    assert w["ddpg actor sb3 missing actor.mu.4.bias"] == {"error": "ValueError: actor.mu.4.bias: missing"}
    assert sum("error" in v for v in w.values()) == 2 * 2 * (12 + 1) + 1


def test_td3_critic_vectors_tensors_and_errors_are_the_parents():
    w = _compare("td3 ")
    assert w["td3 critic sb3 reference flatten"]["flat"][0] == [64202] and w["td3 critic_target tool sb3 flatten"]["flat"][0] == [136706]
    assert "expected shape (200, 8) or (256, 8), got (200, 9)" in w["td3 critic sb3 reference reshaped critic.qf1.0.weight"]["error"]
    assert "mixes the widths of two architectures of the critics" in w["td3 critic tool mixed widths"]["error"]
    assert "expected 64202 or 136706 parameters" in w["td3 critic sb3 sb3 wrong length"]["error"]
    assert sum("error" in v for v in w.values()) == 2 * 2 * (24 + 1) + 2 + 3


def test_sac_actor_vectors_tensors_and_errors_are_the_parents():
    w = _compare("sac ")
    assert w["sac sb3 reference flatten"]["flat"][0] == [63105] and w["sac tool sb3 flatten"]["flat"][0] == [68613]
    assert w["sac sb3 sb3 missing actor.mu.bias"] == {"error": "ValueError: actor.mu.bias: missing"}
    assert w["sac sb3 mixed widths"]["error"].startswith("ValueError: actor.latent_pi.0.weight: shape (256, 6) mixes")
    assert "expected 63105 or 68613 elements" in w["sac tool reference wrong length"]["error"]
    assert [t[:2] for t in w["sac sb3 reference unflatten"]["tensors"]][-1] == ["log_ent_coef", [1]]
    assert sum("error" in v for v in w.values()) == 2 * 2 * (18 + 1) + 2 + 2


def test_quant_actor_flat_vectors_and_errors_are_the_parents():
    w = _compare("quant ")
    served = [k for k, v in w.items() if "flat" in v]
    assert sorted(served) == sorted(["quant ddpg reference dict", "quant ddpg reference flat"] +
                                    [f"quant sac {a} given {a} {how}" for a in ("reference", "sb3") for how in ("dict", "flat", "flat without log_ent_coef")])
    assert w["quant ddpg reference dict"]["flat"][:2] == [[62702], "float64"] and w["quant sac sb3 given sb3 dict"]["flat"][:2] == [[68098], "float64"]
    for how in ("dict", "flat", "flat without log_ent_coef"):   # log_ent_coef and the log_std head are dropped either way
        assert w[f"quant sac reference given reference {how}"] == w["quant sac reference given reference dict"]
    assert "pass net_arch='sb3'" in w["quant sac reference given sb3 dict"]["error"] and "pass net_arch='reference'" in w["quant sac sb3 given reference flat"]["error"]
    assert "head must be 'ddpg' or 'sac'" in w["quant bad head"]["error"] and "net_arch must be 'reference' or 'sb3'" in w["quant bad net_arch"]["error"]
