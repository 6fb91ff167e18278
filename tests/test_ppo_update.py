"""CPU: the PPO update's C ABI (include/auv_hip.h, auv_ppo_*) is declared, bound and exported; the two new structs have the header's
layout; the flat parameter vector is as long as the torch module's; arguments are refused before any device call."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from gym_auv_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
NEW = ["auv_ppo_param_floats", "auv_ppo_create", "auv_ppo_destroy", "auv_ppo_load", "auv_ppo_attach_policy", "auv_ppo_grad", "auv_ppo_adam"]


def test_exports_are_declared_bound_and_present_and_the_abi_version_stays():
    lib = _capi.load_library()
    hdr = open(os.path.join(ROOT, "include", "auv_hip.h")).read()
    for name in NEW:
        assert name in _capi.EXPORTED_SYMBOLS and name + "(" in hdr, name
        assert getattr(lib, name).argtypes is not None, name
    assert _capi.ABI_VERSION == 5 and lib.auv_abi_version() == 5
    assert "scripts/run.py:332-357" in hdr[hdr.index("the PPO update"):]


def test_struct_layouts_match_the_header(tmp_path):
    fields = [("auv_ppo_batch_t", f[0], _capi.AuvPpoBatch) for f in _capi.AuvPpoBatch._fields_]
    fields += [("auv_ppo_adam_t", f[0], _capi.AuvPpoAdam) for f in _capi.AuvPpoAdam._fields_]
    src = tmp_path / "layout.c"
    body = 'printf("%zu %zu\\n", sizeof(auv_ppo_batch_t), sizeof(auv_ppo_adam_t));\n'
    body += "".join('printf("%%zu\\n", offsetof(%s, %s));\n' % (t, f) for t, f, _ in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){%sreturn 0;}\n' % (os.path.join(ROOT, "include", "auv_hip.h"), body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).split()
    assert (C.sizeof(_capi.AuvPpoBatch), C.sizeof(_capi.AuvPpoAdam)) == (int(out[0]), int(out[1])) == (72, 56)
    for (t, f, cls), off in zip(fields, out[2:]):
        assert getattr(cls, f).offset == int(off), (t, f)


@pytest.mark.parametrize("obs_dim", [6, 15, 186])
def test_param_floats_is_the_torch_modules_parameter_count(obs_dim):
    import ppo
    net = ppo.ActorCritic(obs_dim)
    lib = _capi.load_library()
    assert lib.auv_ppo_param_floats(obs_dim) == sum(p.numel() for p in net.parameters())
    assert lib.auv_ppo_param_floats(0) == 0 and lib.auv_ppo_param_floats(-3) == 0
    # the flat layout is the order the module yields its parameters in, log_std last
    names = [n for n, _ in list(net.pi.named_parameters())] + [n for n, _ in list(net.v.named_parameters())]
    assert names == ["0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias", "6.weight", "6.bias"] * 2


def test_arguments_are_refused_before_any_device_call():
    lib = _capi.load_library()
    h = C.c_void_p()
    one = C.c_void_p(16)            # (a non-null pointer that is never dereferenced: every call below is refused first)
    bad = [lib.auv_ppo_create(0, 186, 64, None), lib.auv_ppo_create(0, 0, 64, C.byref(h)), lib.auv_ppo_create(0, -1, 64, C.byref(h)),
           lib.auv_ppo_create(0, 186, 0, C.byref(h)), lib.auv_ppo_create(0, 1 << 20, 64, C.byref(h)), lib.auv_ppo_create(-1, 186, 64, C.byref(h)),
           lib.auv_ppo_load(None, one, None), lib.auv_ppo_attach_policy(None, one),
           lib.auv_ppo_grad(None, C.byref(_capi.AuvPpoBatch()), one, one, None),
           lib.auv_ppo_adam(None, one, one, one, one, C.byref(_capi.AuvPpoAdam()), one, None)]
    assert bad == [-1] * len(bad), bad
    assert h.value is None
    assert b"auv_ppo_adam" in lib.auv_last_error()
    lib.auv_ppo_destroy(None)       # (a no-op)
