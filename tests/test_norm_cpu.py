"""crl_norm without a GPU: the option checks (made before the device is touched), the struct size, and NormalizedEnv's protocol forwarding."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def crl():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "cleanrl.jl_amd", "libcleanrl_hip.so")):
        g.build()
    import cleanrl_jl_amd as crl
    return crl


@pytest.mark.parametrize("kw,msg", [
    (dict(num_envs=0), "num_envs must be in 1..1048576"), (dict(num_envs=(1 << 20) + 1), "num_envs must be in 1..1048576"),
    (dict(obs_dim=0), "obs_dim must be in 1..64"), (dict(obs_dim=65), "obs_dim must be in 1..64"),
    (dict(gamma=-0.1), "gamma must be in \\[0, 1\\]"), (dict(gamma=1.5), "gamma must be in \\[0, 1\\]"), (dict(gamma=float("nan")), "gamma must be"),
    (dict(epsilon=0.0), "epsilon must be positive"), (dict(clip_obs=0.0), "clip_obs must be positive"), (dict(clip_reward=-1.0), "clip_reward must be positive")])
def test_every_option_check_names_its_field(crl, kw, msg):
    L = crl._lib
    assert C.sizeof(L.NormOptions) == 48
    with pytest.raises(L.CrlError, match="crl_norm_create: " + msg):
        L.Normalizer(L.NormOptions(**(dict(num_envs=8, obs_dim=3) | kw)))


class Stub:
    num_envs, obs_dim = 8, 3
    def reset(self): pass
    def step(self, action): pass


def test_normalized_env_forwards_the_protocol(crl):
    disc, cont = Stub(), Stub()
    disc.n_act, disc.stream = 2, 0x1000
    cont.act_dim, cont.on_device, cont.action = 1, True, 0x2000
    d, c = crl.NormalizedEnv(disc), crl.NormalizedEnv(cont, stream=0x3000)
    assert (d.n_act, d.stream, d.training) == (2, 0x1000, True) and not hasattr(d, "act_dim") and not hasattr(d, "on_device")
    assert (c.act_dim, c.on_device, c.action, c.stream) == (1, True, 0x2000, 0x3000) and not hasattr(c, "n_act")
    assert (c.num_envs, c.obs_dim) == (8, 3) and callable(c.episode_stats)
    with pytest.raises(TypeError, match="has no `stream`"):
        crl.NormalizedEnv(cont)
    with pytest.raises(TypeError, match="has no `num_envs`"):
        crl.NormalizedEnv(object(), stream=1)
