#!/usr/bin/env python3
"""The fused update at the reference's widths through this build's library and through ANOTHER build of it (say the parent commit's,
built beside this one), in ONE process, raw ctypes on both (the other build need not export what this binding declares):
(1) bits of the flat gradient, the statistics row, the clone gradients (nll, mse) and theta / m / v after three PPO steps and three clone
steps more, obs_dim 6 and 186, B = 4096 of 5000 rows, fixed seeds; (2) step time of both at B = 16384, obs_dim 186, alternating passes
(HIP events, 10 warm-up steps, the median of 60).  One JSON line per record, to stdout and to --out.

    python tools/ppo_update_vs_build.py /path/to/other/libauv_hip.so --out profiles/ppo_update_arch/bits_vs_parent.jsonl
"""
import ctypes as C
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from gym_auv_amd._capi import AuvPpoAdam, AuvPpoBatch, AuvPpoCloneBatch  # noqa: E402

DEV = "cuda:0"
PATHS = {"new": os.path.join(ROOT, "gym_auv_amd", "csrc", "libauv_hip.so"), "parent": None}    # parent: the other build, from the command line


def load(path):
    lib = C.CDLL(path)
    vp, i32 = C.c_void_p, C.c_int32
    lib.auv_ppo_param_floats.restype, lib.auv_ppo_param_floats.argtypes = C.c_size_t, [i32]
    lib.auv_ppo_create.restype, lib.auv_ppo_create.argtypes = C.c_int, [i32, i32, i32, C.POINTER(vp)]
    lib.auv_ppo_destroy.restype, lib.auv_ppo_destroy.argtypes = None, [vp]
    lib.auv_ppo_load.restype, lib.auv_ppo_load.argtypes = C.c_int, [vp, vp, vp]
    lib.auv_ppo_grad.restype, lib.auv_ppo_grad.argtypes = C.c_int, [vp, C.POINTER(AuvPpoBatch), vp, vp, vp]
    lib.auv_ppo_grad_clone.restype, lib.auv_ppo_grad_clone.argtypes = C.c_int, [vp, C.POINTER(AuvPpoCloneBatch), vp, vp, vp]
    lib.auv_ppo_adam.restype, lib.auv_ppo_adam.argtypes = C.c_int, [vp, vp, vp, vp, vp, C.POINTER(AuvPpoAdam), vp, vp]
    lib.auv_last_error.restype = C.c_char_p
    return lib


class Upd:
    def __init__(self, lib, theta0, obs_dim, max_batch):
        self.lib = lib
        n = int(lib.auv_ppo_param_floats(obs_dim))
        assert n == theta0.numel()
        self.theta, self.m, self.v, self.g = theta0.clone(), torch.zeros_like(theta0), torch.zeros_like(theta0), torch.zeros_like(theta0)
        self.row = torch.zeros(10, device=DEV)
        self.t = 0
        h = C.c_void_p()
        self.ok(lib.auv_ppo_create(0, obs_dim, max_batch, C.byref(h)))
        self.h = h
        self.ok(lib.auv_ppo_load(h, self.theta.data_ptr(), None))

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(self.lib.auv_last_error().decode())

    def grad(self, O, A, LP, ADV, RET, idx):
        b = AuvPpoBatch(O.data_ptr(), A.data_ptr(), LP.data_ptr(), ADV.data_ptr(), RET.data_ptr(), idx.data_ptr(), idx.numel(), O.shape[0], 0.2, 0.5, 0.01)
        self.ok(self.lib.auv_ppo_grad(self.h, C.byref(b), self.g.data_ptr(), self.row.data_ptr(), None))

    def clone_grad(self, O, A, RET, W, idx, kind):
        b = AuvPpoCloneBatch(O.data_ptr(), A.data_ptr(), RET.data_ptr(), W.data_ptr(), idx.data_ptr(), idx.numel(), O.shape[0], kind, 0.5, 0.01)
        self.ok(self.lib.auv_ppo_grad_clone(self.h, C.byref(b), self.g.data_ptr(), self.row.data_ptr(), None))

    def adam(self):
        self.t += 1
        a = AuvPpoAdam(2e-4, 0.9, 0.999, 1e-8, 1.0 - 0.9 ** self.t, 1.0 - 0.999 ** self.t, 0.5, 0.5)
        self.ok(self.lib.auv_ppo_adam(self.h, self.theta.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.g.data_ptr(), C.byref(a),
                                      self.row[8:].data_ptr(), None))

    def close(self):
        torch.cuda.synchronize()
        self.lib.auv_ppo_destroy(self.h)


def rows(obs_dim, n_rows, seed):
    import ppo
    torch.manual_seed(seed)
    net = ppo.ActorCritic(obs_dim).to(DEV)
    theta = torch.cat([p.detach().reshape(-1) for p in list(net.pi.parameters()) + list(net.v.parameters()) + [net.log_std]]).contiguous()
    O, A = torch.randn(n_rows, obs_dim, device=DEV), 0.5 * torch.randn(n_rows, 2, device=DEV)
    with torch.no_grad():
        LP = (net.log_prob(net.pi(O), A) + 0.1 * torch.randn(n_rows, device=DEV)).contiguous()
    ADV, RET, W = torch.randn(n_rows, device=DEV), torch.randn(n_rows, device=DEV), 2.0 * torch.rand(n_rows, device=DEV)
    return theta, (O, A, LP, ADV, RET), (O, A, RET, W)


def bits(libs, out):
    for obs_dim in (6, 186):
        theta, data, cdata = rows(obs_dim, 5000, 1)
        idx = torch.randperm(5000, device=DEV)[:4096].contiguous()
        got = {}
        for name, lib in libs.items():
            r = {}
            u = Upd(lib, theta, obs_dim, 4096)
            u.grad(*data, idx)
            r["ppo_grad"], r["ppo_stats"] = u.g.clone(), u.row[:8].clone()
            for kind in (0, 1):
                u.clone_grad(*cdata, idx, kind)
                r["clone%d_grad" % kind], r["clone%d_stats" % kind] = u.g.clone(), u.row[:8].clone()
            for k in range(3):
                u.grad(*data, idx)
                u.adam()
            r["ppo_theta3"], r["ppo_m3"], r["ppo_v3"] = u.theta.clone(), u.m.clone(), u.v.clone()
            for k in range(3):
                u.clone_grad(*cdata, idx, 0)
                u.adam()
            r["clone_theta6"] = u.theta.clone()
            u.close()
            got[name] = r
        for key in got["new"]:
            a, b = got["new"][key], got["parent"][key]
            rec = dict(kind="bits", obs_dim=obs_dim, B=4096, what=key, elements=a.numel(), equal=bool(torch.equal(a, b)),
                       nonzero=int((a != 0).sum()), max_abs_diff=float((a.double() - b.double()).abs().max()))
            out(rec)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def times(libs, out, passes=4):
    obs_dim, B = 186, 16384
    theta, data, cdata = rows(obs_dim, 131072, 0)
    idx = torch.randperm(131072, device=DEV)[:B].contiguous()
    us = {name: Upd(lib, theta, obs_dim, B) for name, lib in libs.items()}

    def ppo_step(u):
        u.grad(*data, idx)
        u.adam()

    def clone_step(u):
        u.clone_grad(*cdata, idx, 0)
        u.adam()
    for k in range(passes):
        for name, u in us.items():
            out(dict(kind="time", lib=name, obs_dim=obs_dim, B=B, **{"pass": k}, ppo_step_ms=timed(lambda: ppo_step(u), 10, 60),
                     clone_step_ms=timed(lambda: clone_step(u), 10, 60)))
    for u in us.values():
        u.close()


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("other", help="the other build of libauv_hip.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_update_arch", "bits_vs_parent.jsonl"))
    a = ap.parse_args()
    PATHS["parent"] = os.path.abspath(a.other)
    libs = {name: load(p) for name, p in PATHS.items()}
    sha = {name: hashlib.sha256(open(p, "rb").read()).hexdigest() for name, p in PATHS.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def out(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
        out(dict(kind="libs", sha256=sha, device=torch.cuda.get_device_name(0),
                 has_create_arch={name: hasattr(lib, "auv_ppo_create_arch") for name, lib in libs.items()}))
        bits(libs, out)
        times(libs, out)
