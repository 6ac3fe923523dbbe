#!/usr/bin/env python3
"""Locate and explain the env-steps whose fp32 result leaves the 1e-4 band (VERDICT r1, next #1a).

Teacher = the kernel source in DOUBLE on the host (tests/hostsim; agrees with oracle/ to 1e-9 per env step, see
tests/test_hostsim_parity.py) or oracle/ itself (--teacher oracle); student = the same source in FLOAT on the host
(--student host) or the HIP kernel (--student gpu, needs a GPU), teacher-forced per env step (tests/parity.py: env_steps).
Every env-step with max |dqpos| > tol is dumped with its pre-step state and replayed substep by substep in double and float
(host builds, tests/parity.py: replay_substeps) to find the first diverging substep and what happened there: contact onset
(a contact list that differs), an active-set difference, the iteration cap, or plain growth (stick-slip).

    python tools/parity_locate.py --env Env03-v2 --envs 1024 --steps 400 --out profiles/r02_parity_outliers_host.json
"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import parity as P  # noqa: E402

GROUPS = {"torso_pos": [0, 1, 2], "torso_quat": [3, 4, 5, 6], "wheel_angles": [7, 8], "block_pos": [9, 10, 11], "block_quat": [12, 13, 14, 15]}


def group_err(dq):
    return {g: float(np.abs(dq[[i for i in idx if i < dq.size]]).max()) for g, idx in GROUPS.items() if idx[0] < dq.size}


def replay(env_id, pre, tol):
    """one env, substep by substep: host double vs host float from the same pre-step state"""
    d, f = P.make("host64", env_id, 1, noise=False), P.make("host32", env_id, 1, noise=False)
    first_jump, trace = P.replay_substeps(d, f, pre, pre["ctrl"], jump_abs=1e-3, jump_ratio=20, floor=1e-7)
    first_over = next((k for k, (e, _) in enumerate(trace) if e > tol), None)
    return dict(first_substep_dqvel_jump=first_jump, first_substep_dqpos_over=first_over,
                final_dqpos=trace[-1][0], final_dqvel=trace[-1][1],
                dqvel_at_jump=None if first_jump is None else trace[first_jump][1],
                dqvel_before_jump=None if not first_jump else trace[first_jump - 1][1])


def contacts_of(env_id, qpos, qvel, tm):
    """contact list of the pre-state as the oracle sees it (body pairs and distances)"""
    o = P.make("oracle", env_id, 1, noise=False)
    o.set_state(qpos[None], qvel[None], None, np.array([tm]))
    fw = o.forward(env=0, ctrl=(float(qvel[6]), float(qvel[7])))
    return [dict(b1=c["body1"], b2=c["body2"], dist=round(float(c["dist"]), 6)) for c in fw["contacts"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="Env03-v2")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--auto-reset", type=int, default=1)
    ap.add_argument("--teacher", choices=["hostdouble", "oracle"], default="hostdouble")
    ap.add_argument("--student", choices=["host", "gpu"], default="host")
    ap.add_argument("--actions", choices=["random", "zero", "policy"], default="random",
                    help="policy = the reference's MuJoCo-trained balance policy (tests/quant_policy.py) acting on the teacher's observations")
    ap.add_argument("--max-dump", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0, help="seed of both simulators' Philox streams and of the action generator (0 = the campaign of profiles/r03_parity_*.json)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r03_parity_outliers.json"))
    a = ap.parse_args()
    n, ar = a.envs, bool(a.auto_reset)
    T = P.make("oracle" if a.teacher == "oracle" else "host64", a.env, n, seed=a.seed, auto_reset=ar, noise=False)
    S = P.make("hip" if a.student == "gpu" else "host32", a.env, n, seed=a.seed, auto_reset=ar, noise=False)
    obs_t = T.reset(); S.reset()
    outl, nsteps, over, excl, worst = [], 0, 0, 0, 0.0
    upright_over, upright_n = 0, 0
    # per coordinate group x {upright, fallen}: max error and number of env-steps above tol
    gstat = {f"{g}/{u}": [0.0, 0] for g in ("robot", "block") for u in ("upright", "fallen")}
    hist = np.zeros(12, dtype=np.int64)  # log10 buckets of the per-env-step error: <1e-10 ... >=1e0
    t0 = time.time()
    for r in P.env_steps(T, S, a.steps, a.actions, np.random.default_rng(1234 + a.seed), obs=obs_t):
        t, act, qs, qt = r.t, r.act, r.post_s[0], r.post_t[0]
        qpos, qvel, warm, tm, aux, xq, xp = (r.pre[k] for k in ("qpos", "qvel", "warm", "time", "aux", "xquat", "xpos"))
        skip = r.skip if ar else np.zeros(n, bool)   # without auto-reset nothing is re-drawn
        e = np.where(skip, 0.0, np.abs(qs - qt).max(axis=1))
        excl += int(skip.sum()); nsteps += n
        worst = max(worst, float(e.max()))
        hist += np.bincount(np.clip(np.floor(np.log10(np.maximum(e[~skip], 1e-11))).astype(int) + 11, 0, 11), minlength=12)
        upright = P.upright(qpos)
        upright_n += int((upright & ~skip).sum()); upright_over += int((e[upright] > a.tol).sum())
        for g, eg in P.group_errors(qpos, np.abs(qs - qt), skip)[1].items():
            gstat[g][0] = max(gstat[g][0], float(eg.max()))
            gstat[g][1] += int((eg > a.tol).sum())
        bad = np.nonzero(e > a.tol)[0]
        over += bad.size
        for i in bad:
            if len(outl) >= a.max_dump:
                break
            ctrl = qvel[i, 6:8] + act[i].astype(np.float64) * 4.0
            rec = dict(env=int(i), step=int(t), max_dqpos=float(e[i]), per_group=group_err(qs[i] - qt[i]),
                       upright=bool(upright[i]), tilt_deg=float(np.degrees(np.arccos(np.clip(P.cos_tilt(qpos[i:i + 1])[0], -1, 1)))),
                       pre=dict(qpos=qpos[i].tolist(), qvel=qvel[i].tolist(), warm=warm[i].tolist(), time=float(tm[i]), ctrl=ctrl.tolist(),
                                aux=aux[i].tolist(), xquat=xq[i].tolist(), xpos=xp[i].tolist(), action=act[i].tolist()),  # (aux / accessor pose / action: what a replay through brs_step needs)
                       contacts_pre=contacts_of(a.env, qpos[i], qvel[i], tm[i]))
            rec["replay_host_double_vs_float"] = replay(a.env, P.outlier_arrays(rec["pre"]), a.tol)
            outl.append(rec)
        if t % 50 == 0:
            print(f"step {t}: worst {worst:.3g}, over {over}/{nsteps} ({time.time() - t0:.0f} s)", flush=True)
    rep = dict(env=a.env, envs=n, steps=a.steps, seed=a.seed, teacher=a.teacher, student=a.student, auto_reset=ar, tol=a.tol, actions=a.actions,
               env_steps=nsteps, excluded=excl, over=over, worst=worst, upright_env_steps=upright_n, upright_over=upright_over,
               per_group={k: dict(max=v[0], over_tol=v[1]) for k, v in gstat.items()},
               log10_error_histogram={f"1e{k - 11}": int(v) for k, v in enumerate(hist)}, outliers=outl)
    json.dump(rep, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in rep.items() if k != "outliers"}, indent=1))
    for r in outl[:12]:
        print(r["env"], r["step"], f"{r['max_dqpos']:.3g}", r["per_group"], "tilt", round(r["tilt_deg"], 1), r["replay_host_double_vs_float"], r["contacts_pre"])


if __name__ == "__main__":
    main()
