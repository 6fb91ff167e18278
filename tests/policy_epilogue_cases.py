"""Inputs the CPU and the GPU tests of the act launch's sampling epilogue and of the advantage kernel share -- TEST TOOLING ONLY
(tests/test_policy_epilogue.py derives and checks the recorded bounds on them and shows that they are not vacuous,
tests/test_gpu_policy_epilogue.py holds the kernels to those bounds on the same inputs).

The rule of every bound (tests/golden/policy_epilogue_bounds.json): 8 x the largest distance of the float32 NumPy restatement
(gym_auv_amd/policy.py) from the float64 one on the inputs below, at least 4 float32 eps x the largest magnitude of the float64 values.
The factor covers the device's logf / cosf / expf and its freedom to contract a * b + c; nothing in it comes from a kernel's output."""
import functools
import json
import os

import numpy as np

from gym_auv_amd import policy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_PATH = os.path.join(ROOT, "tests", "golden", "policy_epilogue_bounds.json")
RULE = "8 x max |float32 restatement - float64| on the inputs of tests/policy_epilogue_cases.py, floor 4 eps32 x max |float64 value|"
f32, f64 = np.float32, np.float64
EPS32 = float(np.finfo(f32).eps)

# ---- the act launches of the GPU test: N = 40 as the slices [0, 24) and [24, 40), two rollouts of T = 3 and their flush launches ----
SEED, OTHER_SEED, CASES_SEED = 5, 6, 20267
N, T, ROLLOUTS = 40, 3, 2
SLICES = [(0, 24), (24, 16)]
LOG_STDS = [(-0.5, -1.1), (0.5, 0.0)]
# (a flush launch samples nothing but moves the generator on: the sampling launches of rollout r run at the steps r (T + 1) + t)
SAMPLE_STEPS = [r * (T + 1) + t for r in range(ROLLOUTS) for t in range(T)]
SEARCH_CHAIN, SEARCH_STEPS = 0, 1 << 16


def launch_noise(seed, step, dtype=f64, chains=(0, 1), row_keyed=False, one_comp=False, swap=False):
    """eps [N, 2] of the launches of `chains` at generator step `step` (rows of other chains: 0).  The three flags are the mutations the
    CPU test shows the bound to catch: the row inside the slice as the key, component 0's draw for both, the two fields swapped."""
    out = np.zeros((N, 2), dtype=dtype)
    comp = np.zeros((1, 2), dtype=np.int64) if one_comp else np.arange(2)[None, :]
    for i in chains:
        lo, cnt = SLICES[i]
        e = np.arange(cnt)[:, None] + (0 if row_keyed else lo)
        h = P.policy_noise_hash(P.chain_seed(seed, i), step, e, comp)
        if swap:
            h = ((h >> np.uint64(40)) << np.uint64(8)) | (((h >> np.uint64(8)) & np.uint64(0xffffff)) << np.uint64(40))
        out[lo:lo + cnt] = P.box_muller(*P.hash_fields(h), dtype=dtype)
    return out


@functools.lru_cache(maxsize=None)
def searched_step():
    """(step, u1): the generator step below 2^16 at which chain SEARCH_CHAIN of SEED draws its smallest u1 over its environments and both
    components (the first such step), and that u1 -- the launch whose eps lies farthest out in the tail."""
    lo, cnt = SLICES[SEARCH_CHAIN]
    steps = np.arange(SEARCH_STEPS)[:, None, None]
    u1, _ = P.policy_noise_fields(P.chain_seed(SEED, SEARCH_CHAIN), steps, lo + np.arange(cnt)[None, :, None], np.arange(2)[None, None, :])
    k = int(np.argmin(u1.reshape(SEARCH_STEPS, -1).min(axis=1)))
    return k, float(u1[k].min())


def noise_inputs(dtype, **mut):
    """eps of every sampling launch of the two rollouts, [len(SAMPLE_STEPS), N, 2], and of the searched launch of chain SEARCH_CHAIN."""
    runs = np.stack([launch_noise(SEED, g, dtype, **mut) for g in SAMPLE_STEPS])
    return runs, launch_noise(SEED, searched_step()[0], dtype, chains=(SEARCH_CHAIN,), **mut)


def _bound(v32, v64):
    v64 = np.asarray(v64, dtype=f64)
    err = float(np.abs(np.asarray(v32).astype(f64) - v64).max())
    return max(8.0 * err, 4.0 * EPS32 * float(np.abs(v64).max()))


def eps_bound():
    a32, b32 = noise_inputs(f32)
    a64, b64 = noise_inputs(f64)
    return _bound(np.concatenate([a32.ravel(), b32.ravel()]), np.concatenate([a64.ravel(), b64.ravel()]))


def sample_inputs(log_std):
    """(mu, eps, log_std) float32: means of the size the test's nets give, uniform in (-1, 1), seeded; the float32 draws of the sampling
    launches; the log-std pair as the float32 parameter holds it."""
    rs = np.random.RandomState(CASES_SEED + LOG_STDS.index(tuple(log_std)))
    mu = rs.uniform(-1.0, 1.0, (len(SAMPLE_STEPS), N, 2)).astype(f32)
    return mu, noise_inputs(f32)[0], np.array(log_std, dtype=f32)


def sample_bounds(log_std):
    """(bound of A, bound of LP): A on (mu, eps), LP on (float32 A, mu) -- as the GPU test forms them from the launch's own mu and eps."""
    mu, eps, ls = sample_inputs(log_std)
    a32 = P.sample_reference(mu, ls, eps, f32)
    assert a32.dtype == f32
    return _bound(a32, P.sample_reference(mu, ls, eps, f64)), _bound(P.logp_reference(a32, mu, ls, f32), P.logp_reference(a32, mu, ls, f64))


# ---- auv_gae ----
GAE_SHAPES = [(1, 1), (1, 257), (5, 255), (5, 256), (64, 257), (512, 65)]          # (T, N)
GAE_PARAMS = [(0.999, 0.98), (1.0, 1.0), (0.99, 0.0), (0.0, 0.95)]                   # (gamma, lam)
GAE_DONES = ["none", "all", "random"]


def gae_inputs(Tn, Nn, dones):
    """R, V, Dn [T, N] and last_v [N], float32, unit scale, seeded by the shape.  "random": done with probability 0.1, and a done forced
    at t = T - 1 for environment 1 and at t = 0 for environment 2 (where N has them)."""
    rs = np.random.RandomState(CASES_SEED + 1000 * Tn + Nn)
    R, V, last_v = (rs.standard_normal(s).astype(f32) for s in ((Tn, Nn), (Tn, Nn), (Nn,)))
    u = rs.uniform(size=(Tn, Nn))
    if dones == "none":
        Dn = np.zeros((Tn, Nn), dtype=f32)
    elif dones == "all":
        Dn = np.ones((Tn, Nn), dtype=f32)
    else:
        Dn = (u < 0.1).astype(f32)
        if Nn > 1:
            Dn[Tn - 1, 1] = 1.0
        if Nn > 2:
            Dn[0, 2] = 1.0
    return R, V, Dn, last_v


def gae_bound(Tn, Nn, gamma, lam, dones):
    R, V, Dn, last_v = gae_inputs(Tn, Nn, dones)
    a32 = P.gae_reference(R, V, Dn, last_v, gamma, lam, f32)[0]
    assert a32.dtype == f32
    return _bound(a32, P.gae_reference(R, V, Dn, last_v, gamma, lam, f64)[0])


def gae_cases():
    return [(Tn, Nn, g, l, d) for Tn, Nn in GAE_SHAPES for g, l in GAE_PARAMS for d in GAE_DONES]


def _key(log_std):
    return "%g,%g" % tuple(log_std)


def computed_bounds():
    step, u1 = searched_step()
    sb = {_key(ls): sample_bounds(ls) for ls in LOG_STDS}
    return {"seed": SEED, "cases_seed": CASES_SEED, "rule": RULE, "searched_step": step, "searched_u1": u1, "eps": eps_bound(),
            "A": {k: v[0] for k, v in sb.items()}, "LP": {k: v[1] for k, v in sb.items()},
            "gae": [{"T": Tn, "N": Nn, "gamma": g, "lam": l, "dones": d, "bound": gae_bound(Tn, Nn, g, l, d)} for Tn, Nn, g, l, d in gae_cases()]}


@functools.lru_cache(maxsize=None)
def recorded():
    rec = json.load(open(BOUNDS_PATH))
    assert rec["seed"] == SEED and rec["cases_seed"] == CASES_SEED and rec["rule"] == RULE
    return rec


def recorded_bound(what, log_std=None):
    """The recorded bound of "eps", or of "A" / "LP" under `log_std`."""
    rec = recorded()
    return float(rec[what]) if log_std is None else float(rec[what][_key(log_std)])


def recorded_gae_bound(Tn, Nn, gamma, lam, dones):
    hit = [c for c in recorded()["gae"] if (c["T"], c["N"], c["gamma"], c["lam"], c["dones"]) == (Tn, Nn, gamma, lam, dones)]
    assert len(hit) == 1, (Tn, Nn, gamma, lam, dones)
    return float(hit[0]["bound"])


if __name__ == "__main__":                         # regenerate the file after a deliberate change of the inputs
    json.dump(computed_bounds(), open(BOUNDS_PATH, "w"), indent=1)
    print(open(BOUNDS_PATH).read())
