"""CPU: the contract loop of the value-terminated plan score (planning.reference_plan_score_terminal) and the ctypes mirror of
auv_policy_eval_t (include/auv_hip.h)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gym_auv_amd import _capi
from gym_auv_amd.planning import reference_plan_score, reference_plan_score_terminal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    np.testing.assert_array_equal(a[1], b[1])


def test_terminal_score_reduces_to_the_plain_score():
    rs = np.random.RandomState(0)
    T, n, group = 7, 24, 4
    rew = rs.randn(T, n).astype(np.float32)
    done = rs.rand(T, n) < 0.1
    term = (rs.randn(n) * 10).astype(np.float32)
    # a zero terminal: s + disc * 0 == s (no score of this record is -0.0)
    _same(reference_plan_score_terminal(rew, done, group, 0.97, np.zeros(n, np.float32)), reference_plan_score(rew, done, group, 0.97))
    # every environment saw a done: the terminal is never read, not even a NaN
    d2 = done.copy()
    d2[T - 1] = True
    _same(reference_plan_score_terminal(rew, d2, group, 0.97, np.full(n, np.nan, np.float32)), reference_plan_score(rew, d2, group, 0.97))
    # without a done it does count
    d3 = np.zeros_like(done)
    s, _ = reference_plan_score_terminal(rew, d3, group, 0.97, term)
    s0, _ = reference_plan_score(rew, d3, group, 0.97)
    assert (s != s0).all()
    with pytest.raises(ValueError):
        reference_plan_score_terminal(rew, done, 5, 0.97, term)
    with pytest.raises(ValueError):
        reference_plan_score_terminal(rew, done, group, 0.97, term[:-1])


def test_terminal_score_by_hand_for_two_steps():
    f = np.float32
    g = f(0.9)
    rew = np.array([[1.5, 2.0, -1.0, 0.25], [0.5, 4.0, 3.0, 8.0]], dtype=np.float32)
    done = np.array([[0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.uint8)
    term = np.array([10.0, 100.0, 1000.0, np.nan], dtype=np.float32)
    s, b = reference_plan_score_terminal(rew, done, 2, 0.9, term)
    disc2 = f(f(1.0) * g) * g                               # the running product after T = 2 multiplications
    want0 = f(f(f(1.5) + f(g * f(0.5))) + f(f(disc2) * f(10.0)))
    assert s[0] == want0                                    # no done: r0 + g r1 + g^2 * terminal
    assert s[1] == f(2.0)                                   # done at t = 0: the first reward alone
    assert s[2] == f(f(-1.0) + f(g * f(3.0)))               # done at t = 1 = T - 1: no terminal
    assert np.isnan(s[3])                                   # no done and a NaN terminal
    assert b.tolist() == [0, 0]                             # 10.05 > 2; a NaN never wins


def test_policy_eval_struct_matches_the_header(tmp_path):
    """sizeof / offsetof from the real header (compiled with gcc) == the ctypes mirror."""
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu\\n", '
                   'sizeof(auv_policy_eval_t), offsetof(auv_policy_eval_t, mu), offsetof(auv_policy_eval_t, ldx), '
                   'offsetof(auv_policy_eval_t, M), offsetof(auv_policy_eval_t, clip_hi));return 0;}\n'
                   % os.path.join(ROOT, "include", "auv_hip.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    size, o_mu, o_ldx, o_m, o_hi = map(int, subprocess.check_output([str(exe)]).split())
    E = _capi.AuvPolicyEval
    assert C.sizeof(E) == size
    assert (E.mu.offset, E.ldx.offset, E.M.offset, E.clip_hi.offset) == (o_mu, o_ldx, o_m, o_hi)


def test_new_exports_are_declared_and_bound():
    assert "auv_policy_eval" in _capi.EXPORTED_SYMBOLS and "auv_plan_score_v" in _capi.EXPORTED_SYMBOLS
    lib = _capi.load_library()
    assert hasattr(lib, "auv_policy_eval") and hasattr(lib, "auv_plan_score_v")
