"""CPU: what the verifications of members against an observation share in pr_disagg_radar_gan_amd/_hourly.py -- the pair check, the
grow-only workspace, and the host half of the four `*_field` drivers, which refuse the same bad arguments before any device call."""
import types

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _hourly as H, _lib, distmap, intensity_scale, sal, verification

FIELDS = (verification.verify_field, intensity_scale.intensity_scale_field, distmap.distmap_field, sal.sal_field)


def test_check_pair():
    obs = (2, 24, 5, 6)
    H.check_pair((3,) + obs, obs)
    H.check_pair(np.broadcast_to(np.float32(0), (4096, 24, 2, 2)).shape, (24, 2, 2))
    with pytest.raises(ValueError, match=r"ens: expected an array or tensor of shape \(S, \.\.\., 24, ny, nx\)"):
        H.check_pair((24, 5, 6), (24, 5, 6))
    with pytest.raises(ValueError, match="members: expected an array"):
        H.check_pair((24, 5, 6), (24, 5, 6), "members")
    with pytest.raises(ValueError, match=r"must lie in 1 \.\. 4096, got 4097"):
        H.check_pair(np.broadcast_to(np.float32(0), (4097, 24, 2, 2)).shape, (24, 2, 2))
    with pytest.raises(ValueError, match=r"ens: expected shape \(S,\) \+ \(2, 24, 5, 6\), got \(3, 2, 24, 5, 7\)"):
        H.check_pair((3, 2, 24, 5, 7), obs)
    with pytest.raises(ValueError, match="expected shape"):
        H.check_pair((3, 24, 5, 6), obs)                            # the day axis is missing


class Words:
    """stands for a workspace of n int64 words: numel() and nothing else"""

    def __init__(self, n):
        self.n = n

    def numel(self):
        return self.n


def test_grow_workspace():
    held = Words(100)
    owner = types.SimpleNamespace(_ws=held)
    assert H.grow_workspace(owner, 800, "meta") is held and owner._ws is held            # exactly enough
    assert H.grow_workspace(owner, 8, "meta") is held and owner._ws is held              # a larger buffer stays
    new = H.grow_workspace(owner, 801, "meta")                                           # a smaller one is replaced
    assert new is owner._ws and new is not held and new.dtype == torch.int64 and new.numel() == 101      # (bytes round up to 8)
    assert H.grow_workspace(owner, 808, "meta") is new
    owner = types.SimpleNamespace(_ws=None)
    assert H.grow_workspace(owner, 1, "meta").numel() == 1 and owner._ws.device.type == "meta"


class NoGenerator:
    ndomain, n_cond_channels = 16, 1


OK = dict(gen=NoGenerator(), observed=np.zeros((24, 20, 30), np.float32), n_scenarios=16, thresholds=(0.1,))
BAD = ((dict(observed=np.zeros((2, 2, 24, 20, 30), np.float32)), "observed must have shape"),
       (dict(observed=torch.zeros(24, 20, 30)), "observed: expected a CUDA tensor or a numpy array"),
       (dict(observed=np.zeros((20, 30), np.float32)), "observed: expected shape"),
       (dict(observed=np.zeros((23, 20, 30), np.float32)), "observed: expected shape"),
       (dict(observed=np.zeros((24, 0, 30), np.float32)), "observed: expected shape"),
       (dict(observed=np.zeros((24, 20, 30), dtype=complex)), "observed: expected an array of numbers"),
       (dict(daily=np.zeros((20, 31), np.float32)), "daily: expected shape"),
       (dict(daily=torch.zeros(1, 20, 30)), "daily: expected shape"),
       (dict(daily=np.zeros((24, 20, 30), np.float32)), "daily: expected shape"),
       (dict(observed=np.zeros((2, 24, 20, 30), np.float32), daily=np.zeros((20, 30), np.float32)), "daily: expected shape"),
       (dict(thresholds=()), "thresholds"), (dict(n_scenarios=0), "number of scenarios"), (dict(n_scenarios=4097), "number of scenarios"),
       (dict(scenario_chunk=0), "scenario_chunk"), (dict(overlap=9), "overlap"), (dict(latent_mode="each"), "latent_mode"),
       (dict(chunk=0), "chunk must be at least 1"), (dict(norm_scale=0.0), "norm_scale"))


@pytest.mark.parametrize("field", FIELDS, ids=lambda f: f.__name__)
def test_the_field_drivers_refuse_the_same_arguments_before_the_device(field):
    for kw, message in BAD:
        with pytest.raises(ValueError, match=message):
            field(**{**OK, **kw})
    if not torch.cuda.is_available():                               # valid arguments reach the device: there is no CPU fallback
        for kw in (dict(), dict(daily=np.zeros((20, 30), np.float32)), dict(observed=np.zeros((2, 24, 20, 30), np.float32))):
            with pytest.raises(_lib.RdganError):
                field(**{**OK, **kw})
