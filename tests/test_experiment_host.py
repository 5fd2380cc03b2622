"""The seed rules of the joint-ensemble experiments as calls, without a GPU: multivariate.multivariate_experiment and
multivariate_ranks.multivariate_rank_experiment run over stubs of the device layer, of the four ensemble makers and of the per-day
scoring functions, which record what they are called with.  Asserted: day d's GAN ensemble is seeded seed + d, RainFARM starts at
member d * n_members, the analog library and the cascade are asked for query d (the library with its query_groups cut to [d:d+1], the
cascade with patch = cascade_patch), k and analog_weights arrive as given, every ensemble is scored against its own day before the
next one is made, the methods come in the order gan, random, rainfarm, analog, cascade -- and the two experiments make the very
same calls."""
import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _experiment, ensemble, multivariate as MV, multivariate_ranks as MR, rainfarm, weights as W
from pr_disagg_radar_gan_amd.analog import AnalogLibrary
from pr_disagg_radar_gan_amd.cascade import CascadeModel

DEVICE_LAYER = (_experiment,)                                                              # the modules whose require_gpu and device_f32 the experiments call
D, M, ND, SEED, SLOPES, K, PATCH = 3, 4, 8, 5, (2.2, 1.3), 7, 8
GROUPS = np.array([11, 12, 13])


class OnDevice(torch.Tensor):
    """a CPU tensor that the host checks take for one on the device"""
    is_cuda = property(lambda self: True)


def fake_device_f32(a, name, device=None):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).as_subclass(OnDevice)


def plain(t):
    return t.as_subclass(torch.Tensor)


class Log:
    """every stub appends here; a maker's ensemble is filled with the (1-based) position of its call among the makers' calls"""

    def __init__(self):
        self.events = []

    def made(self, *call):
        self.events.append(call)
        return float(len(self.makers()))

    def makers(self):
        return [e for e in self.events if e[0] not in ("score", "score_shared", "require_gpu")]


class StubLibrary(AnalogLibrary):
    def __init__(self, log):
        self.plane_shape, self.log = (ND, ND), log

    def generate(self, cond, n_members, k=10, seed=0, weights="rank", query_groups=None, first_member=0, return_picks=False, first_query=0):
        tag = self.log.made("analog", tuple(cond.shape), float(cond[0, 0, 0]), n_members, k, seed, weights, first_query,
                            None if query_groups is None else np.asarray(query_groups).tolist(), first_member)
        return torch.full((1, n_members, 24, ND, ND), tag)


class StubCascade(CascadeModel):
    def __init__(self, log):
        self.log = log

    def generate(self, cond, n_members, seed=0, first_member=0, first_query=0, patch=1, return_units=False, out=None):
        tag = self.log.made("cascade", tuple(cond.shape), float(cond[0, 0, 0]), n_members, seed, first_query, patch, first_member)
        return torch.full((1, n_members, 24, ND, ND), tag)


def reals_and_climatology():
    reals = np.stack([np.full((24, ND, ND), d + 1.0, np.float32) for d in range(D)])       # day d holds d + 1 everywhere: its daily sum is 24 (d + 1)
    return reals, np.zeros((6, 24, ND, ND), np.float32)


def gan_scale(d):
    dsum = torch.full((ND, ND), 24.0 * (d + 1))
    return float((dsum / W.NORM_SCALE * W.NORM_SCALE)[0, 0])


def run(monkeypatch, experiment, per_day_scores, **own):
    """-> (result, log).  per_day_scores: the stubs of the module's scoring functions, {name: factory(log)}"""
    log = Log()
    for mod in DEVICE_LAYER:
        monkeypatch.setattr(mod, "require_gpu", lambda: log.events.append(("require_gpu",)) and None)
        monkeypatch.setattr(mod, "device_f32", fake_device_f32)

    def generate_ensemble_device(gen, cond_norm, n_members, chunk=1024, seed=None, latent=None):
        assert isinstance(cond_norm, np.ndarray) and cond_norm.shape == (ND, ND, 1)
        return torch.full((n_members, 24, ND, ND), log.made("gan", gen, float(cond_norm[0, 0, 0]), n_members, seed))

    def downscale_device(precip, alpha, beta, n_members=None, seed=None, uniforms=None, first_member=0):
        return torch.full((n_members, 24, ND, ND), log.made("rainfarm", tuple(precip.shape), float(precip[0, 0]), alpha, beta, n_members, seed,
                                                           first_member, uniforms))

    monkeypatch.setattr(ensemble, "generate_ensemble_device", generate_ensemble_device)
    monkeypatch.setattr(rainfarm, "downscale_device", downscale_device)
    for (mod, name), factory in per_day_scores.items():
        monkeypatch.setattr(mod, name, factory(log))
    reals, clim = reals_and_climatology()
    res = experiment("the generator", reals, clim, slopes=SLOPES, library=StubLibrary(log), n_members=M, seed=SEED, k=K, analog_weights="uniform",
                     query_groups=GROUPS, cascade=StubCascade(log), cascade_patch=PATCH, **own)
    log.events = [e for e in log.events if e != ("require_gpu",)]
    return res, log


def scored(log, name, ens, obs):
    """what a scoring stub records: which maker's call the ensemble came from and which day it meets"""
    ens, obs = plain(ens), plain(obs)
    if obs.dim() == 4:
        log.events.append(("score_shared", name, tuple(ens.shape), tuple(obs.shape)))
        return int(obs.shape[0])
    assert tuple(ens.shape) == (M, 24, ND, ND) and tuple(obs.shape) == (24, ND, ND) and bool((ens == ens[0, 0, 0, 0]).all())
    log.events.append(("score", name, float(ens[0, 0, 0, 0]), int(obs[0, 0, 0]) - 1))
    return 1


def score_stubs():
    def energy(log):
        return lambda ens, obs, fair=False: torch.zeros(scored(log, "es", ens, obs), dtype=torch.float64)

    def variogram(log):
        return lambda ens, obs, **kw: torch.zeros(scored(log, "vs", ens, obs), dtype=torch.float64)

    return {(MV, "energy_score"): energy, (MV, "variogram_score"): variogram}


def rank_stubs():
    def ranks(log):
        def multivariate_ranks(ens, obs, kinds=MR.KINDS, by_hour=False, pool=1):
            n = scored(log, "ranks", ens, obs)
            zeros = {k: np.zeros(n, np.int64) for k in kinds}
            return MR.MultivariateRanks(tuple(kinds), int(ens.shape[0]), dict(zeros), dict(zeros), {k: np.ones(n, np.int64) for k in kinds})
        return multivariate_ranks

    return {(MR, "multivariate_ranks"): ranks}


def expected_makers():
    """the seed rules, written out"""
    calls = [("gan", "the generator", 24.0 * (d + 1) / W.NORM_SCALE, M, SEED + d) for d in range(D)]
    calls += [("rainfarm", (ND, ND), 24.0 * (d + 1), SLOPES[0], SLOPES[1], M, SEED, d * M, None) for d in range(D)]
    calls += [("analog", (1, ND, ND), 24.0 * (d + 1), M, K, SEED, "uniform", d, [int(GROUPS[d])], 0) for d in range(D)]
    calls += [("cascade", (1, ND, ND), 24.0 * (d + 1), M, SEED, d, PATCH, 0) for d in range(D)]
    return calls


def expected_events(score_names):
    """every ensemble meets its own day right after it is made; the shared climatology comes between the GAN and RainFARM"""
    out, made = [], 0
    for method, call in zip(("gan",) * D + ("rainfarm",) * D + ("analog",) * D + ("cascade",) * D, expected_makers()):
        d = made % D
        made += 1
        out.append(call)
        out += [("score", s, made * (gan_scale(d) if method == "gan" else 1.0), d) for s in score_names]
        if made == D:
            out += [("score_shared", s, (6, 24, ND, ND), (D, 24, ND, ND)) for s in score_names]
    return out


def close(a, b):
    """two event lists: equal, floats to 1e-6 relative (a daily sum over 127.4 is an fp32 quotient)"""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if len(x) != len(y):
            return False
        for u, v in zip(x, y):
            if isinstance(u, float) and isinstance(v, float):
                if abs(u - v) > 1e-6 * abs(v):
                    return False
            elif u != v:
                return False
    return True


def test_both_experiments_make_the_same_ensembles_by_the_seed_rules(monkeypatch):
    scores, log_s = run(monkeypatch, MV.multivariate_experiment, score_stubs())
    ranks, log_r = run(monkeypatch, MR.multivariate_rank_experiment, rank_stubs(), kinds=("average", "mst"), pool=2)
    assert log_s.makers() == log_r.makers()                                                # the two experiments see the same members
    assert close(log_s.makers(), expected_makers()), log_s.makers()
    assert close(log_s.events, expected_events(("es", "vs"))), log_s.events
    assert close(log_r.events, expected_events(("ranks",))), log_r.events
    order = ["gan", "random", "rainfarm", "analog", "cascade"]
    assert list(scores.es) == list(scores.vs) == list(ranks) == order
    assert all(v.shape == (D,) and v.dtype == np.float64 for t in (scores.es, scores.vs) for v in t.values())
    assert all(r.kinds == ("average", "mst") and r.below["mst"].shape == (D,) for r in ranks.values())
    assert ranks["gan"].n_members == M and ranks["random"].n_members == 6


def test_the_optional_methods_are_left_out_and_the_defaults_passed_on(monkeypatch):
    for experiment, stubs, names in ((MV.multivariate_experiment, score_stubs(), ("es", "vs")), (MR.multivariate_rank_experiment, rank_stubs(), ("ranks",))):
        log = Log()
        for mod in DEVICE_LAYER:
            monkeypatch.setattr(mod, "require_gpu", lambda: None)
            monkeypatch.setattr(mod, "device_f32", fake_device_f32)
        monkeypatch.setattr(ensemble, "generate_ensemble_device",
                            lambda gen, cond, n, chunk=1024, seed=None, latent=None: torch.full((n, 24, ND, ND), log.made("gan", gen, float(cond[0, 0, 0]), n, seed)))
        for (mod, name), factory in stubs.items():
            monkeypatch.setattr(mod, name, factory(log))
        reals, clim = reals_and_climatology()
        res = experiment("g", reals, clim, n_members=M, library=StubLibrary(log))           # seed 0, k 10, rank weights, no groups
        assert list(res.es if hasattr(res, "es") else res) == ["gan", "random", "analog"]
        makers = log.makers()
        assert [c[0] for c in makers] == ["gan"] * D + ["analog"] * D
        assert [c[4] for c in makers[:D]] == [0, 1, 2]
        assert makers[D:] == [("analog", (1, ND, ND), 24.0 * (d + 1), M, 10, 0, "rank", d, None, 0) for d in range(D)]


def test_a_bad_roster_is_refused_before_any_device_call(monkeypatch):
    """the roster's ValueErrors come before require_gpu, in both experiments"""
    def no_device():
        raise AssertionError("the device was asked for")
    for mod in DEVICE_LAYER:
        monkeypatch.setattr(mod, "require_gpu", no_device)
        monkeypatch.setattr(mod, "device_f32", lambda *a, **k: no_device())
    reals, clim = reals_and_climatology()
    log = Log()
    for experiment in (MV.multivariate_experiment, MR.multivariate_rank_experiment):
        for kw in (dict(slopes=(1.0,)), dict(library="days"), dict(query_groups=GROUPS), dict(library=StubLibrary(log), query_groups=GROUPS[:2]),
                   dict(cascade="model"), dict(cascade=StubCascade(log), cascade_patch=0), dict(n_members=0), dict(n_members=True), dict(seed=-1),
                   dict(seed=1.5)):
            with pytest.raises(ValueError):
                experiment("g", reals, clim, **kw)
        for bad_reals, bad_clim in ((reals[0], clim), (reals[:, :, :, :4], clim[:, :, :, :4]), (reals, clim[:, :, :4, :4]), (reals, clim[:, :23])):
            with pytest.raises(ValueError):
                experiment("g", bad_reals, bad_clim)
    assert log.events == []
