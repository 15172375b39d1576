"""The device-resident external-env path (crl_rollout_act_device & co.) as far as it can be checked without a GPU: the five exports exist in the header,
the binding table and the library; the Handle wrappers validate pointer arguments before the library is touched; ppo / train_external refuse what they
cannot run; the Julia shell calls the new entry points with the header's arity."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["crl_ppo_stream", "crl_rollout_act_device", "crl_rollout_record_device", "crl_env_step_device", "crl_ppo_update"]


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as m
    m._lib.load()
    return m


def _header():
    return open(os.path.join(ROOT, "include", "cleanrl_hip.h")).read()


def test_five_exports_in_header_table_and_library(crl):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = crl._lib.load()
    for name in NEW:
        assert re.search(r"^int32_t %s\(" % name, hdr, re.M), f"{name} is not declared in the header"
        assert name in crl._lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is not None


def test_handle_has_the_five_methods(crl):
    H = crl._lib.Handle
    assert isinstance(H.stream, property)
    for m in ("act_device", "record_device", "env_step_device", "update"):
        assert callable(getattr(H, m))


class _NoDevice:
    """a Handle whose library pointer must never be used: any call through it would dereference NULL inside the library"""


@pytest.mark.parametrize("bad,exc", [(0, ValueError), (None, ValueError), (np.zeros(4, np.float32), TypeError), (1.5, TypeError)],
                         ids=["zero", "none", "numpy", "float"])
def test_pointer_validation_raises_before_any_device_call(crl, monkeypatch, bad, exc):
    L = crl._lib
    touched = []
    monkeypatch.setattr(L, "load", lambda: touched.append(1) or (_ for _ in ()).throw(AssertionError("the library was touched")))
    h = object.__new__(L.Handle)     # no crl_ppo_create: there is no device here, and validation must not need one
    h._h = None
    good = 0x1000
    calls = [lambda: h.act_device(0, bad, good, good), lambda: h.act_device(0, good, bad, good), lambda: h.act_device(0, good, good, bad),
             lambda: h.record_device(0, bad, good, good), lambda: h.record_device(0, good, bad, good), lambda: h.record_device(0, good, good, bad),
             lambda: h.env_step_device(bad, 0, good, good, good), lambda: h.env_step_device(good, 0, good, bad, good),
             lambda: h.env_step_device(good, 0, good, good, bad)]
    for c in calls:
        with pytest.raises(exc):
            c()
    if exc is TypeError:             # an optional pointer accepts None / 0, nothing else that is not a pointer
        with pytest.raises(TypeError):
            h.env_step_device(good, 0, bad, good, good)
        with pytest.raises(TypeError):
            h.act_device(0, good, good, good, peer_stream=bad)
    assert not touched
    h._h = None


def test_devptr_accepts_ints_and_data_ptr_objects(crl):
    class T:
        def data_ptr(self):
            return 0x7F0000001000
    assert crl._lib.devptr(0x1000) == 0x1000 and crl._lib.devptr(T()) == 0x7F0000001000
    assert crl._lib.devptr(None, optional=True) is None and crl._lib.devptr(0, optional=True) is None
    with pytest.raises(TypeError):
        crl._lib.devptr(True)


def test_ppo_with_a_non_env_object_names_the_missing_attribute(crl, monkeypatch):
    monkeypatch.setattr(crl._lib.Handle, "__init__", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a handle was created")))
    with pytest.raises(TypeError, match="num_envs"):
        crl.ppo(crl.PPOConfig(), env=object())

    class Half:
        num_envs, obs_dim, n_act = 4, 4, 2

        def reset(self):
            pass
    with pytest.raises(TypeError, match="step"):
        crl.ppo(crl.PPOConfig(), env=Half())


def test_train_external_rejects_eval_every(crl):
    with pytest.raises(ValueError, match="eval_every"):
        crl.train_external(None, object(), eval_every=1)
    with pytest.raises(ValueError, match="eval_every"):
        class E:
            num_envs, obs_dim, n_act = 4, 4, 2
            reset = step = staticmethod(lambda *a: None)
        crl.ppo(crl.PPOConfig(), env=E(), eval_every=1)


def test_julia_shell_calls_the_new_entry_points_with_the_headers_arity():
    jl = open(os.path.join(ROOT, "julia", "CleanRLHip.jl")).read()
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("crl_rollout_act_device", "crl_rollout_record_device", "crl_ppo_update", "crl_ppo_stream"):
        decl = re.search(r"^int32_t %s\((.*?)\);" % name, hdr, re.M | re.S).group(1)
        arity = len([a for a in decl.split(",") if a.strip()])
        m = re.search(r"ccall\(\(:%s, libcrl\), Int32, \((.*?)\),\s*\n?\s*a\.h" % name, jl, re.S)
        assert m, f"{name} is not ccalled in the Julia shell"
        types = [t for t in re.split(r",\s*", m.group(1).strip()) if t]
        assert len(types) == arity, (name, types, arity)
        assert types[0] == "Ptr{Cvoid}"
    assert "function ppo_external(config::PPOConfig, env;" in jl
