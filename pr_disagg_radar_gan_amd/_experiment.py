"""The roster of the joint-ensemble experiments: which methods compete over the real days, how each makes day
d's ensemble -- the SEED RULES, written here and nowhere else -- and the loop that keeps one ensemble alive at a time.
multivariate.multivariate_experiment scores these ensembles, multivariate_ranks.multivariate_rank_experiment ranks the observation
among them; a new experiment takes its competitors from competing_methods and sees the same members.  Host code: no kernels."""
import numpy as np

from . import ensemble, rainfarm
from . import weights as W
from ._dev import device_f32, whole_number
from ._hourly import MAX_PLANE, NHOURS, check_reals
from .analog import AnalogLibrary
from .cascade import CascadeModel
from .engine import require_gpu


def for_each_day(make_ensemble, reals, per_day):
    """reals (D, 24, ny, nx), numpy or CUDA; make_ensemble(d) -> day d's (m, 24, ny, nx) ensemble, handed to per_day(d, ens,
    reals[d]) and dropped before the next one is made: the m 24 ny nx floats exist for one day at a time.  -> [per_day's results]"""
    if not callable(make_ensemble):
        raise ValueError("make_ensemble must be callable")
    shape = check_reals(reals)
    require_gpu()
    reals = device_f32(reals, "reals")
    out = []
    for d in range(shape[0]):
        ens = make_ensemble(d)
        out.append(per_day(d, ens, reals[d]))
        del ens
    return out


def gan_ensemble(gen, real, n_members, seed=None, norm_scale=W.NORM_SCALE):
    """The generator's ensemble for one real day (24, nd, nd) on the host, in mm/h: the fractions of
    ensemble.generate_ensemble_device times the condition, as crps_experiment.crps_for_days scales them"""
    dsum = real.sum(0)
    fractions = ensemble.generate_ensemble_device(gen, (dsum / norm_scale).numpy()[..., None], n_members, seed=seed)
    return fractions * (dsum / norm_scale * norm_scale).to(fractions.device)


class Roster:
    """What competing_methods returns: reals, the real days on the device; climatology, as given (run moves it); n_members; makers,
    {name: make_ensemble(d)} in the order gan, rainfarm, analog, cascade, the optional ones where the experiment has them."""

    def __init__(self, reals, climatology, n_members, makers):
        self.reals, self.climatology, self.n_members, self.makers = reals, climatology, n_members, makers

    def run(self, for_days, shared):
        """{method: result} in the order gan, random, rainfarm, analog, cascade: for_days(make_ensemble), but shared(climatology,
        reals) for "random", the fixed climatological ensemble, which goes to the device only once the GAN's days are done"""
        out = {"gan": for_days(self.makers["gan"])}
        out["random"] = shared(device_f32(self.climatology, "climatology", self.reals.device), self.reals)
        out.update((name, for_days(make)) for name, make in self.makers.items() if name != "gan")
        return out


def competing_methods(gen, reals_precip, climatology, *, max_members, slopes=None, library=None, n_members=1000, seed=0, k=10,
                      analog_weights="rank", query_groups=None, cascade=None, cascade_patch=1):
    """The competitors of an experiment over the real days reals_precip (D, 24, nd, nd) mm/h -> Roster.  Every argument is checked
    before the first device call; max_members bounds n_members and the climatology (n, 24, nd, nd).  Day d's m = n_members members:
      gan        gan_ensemble by the device generator seeded seed + d (crps_experiment.crps_for_days)
      rainfarm   with slopes = (alpha, beta): the members d m .. (d + 1) m - 1 of the counter RNG (rainfarm_crps_for_days)
      analog     with library = an AnalogLibrary: library.generate(daily sum of day d, m, k, seed, analog_weights, first_query=d),
                 query_groups (D,) leaving the library's days of the same group out
      cascade    with cascade = a CascadeModel: cascade.generate(daily sum of day d, m, seed, first_query=d, patch=cascade_patch)"""
    shape = check_reals(reals_precip, "reals_precip")
    cs = check_reals(climatology, "climatology")
    if shape[2] != shape[3] or cs[1:] != shape[1:] or cs[0] > max_members:
        raise ValueError(f"reals_precip (D, {NHOURS}, nd, nd) and climatology (n <= {max_members}, {NHOURS}, nd, nd) expected, got {shape} and {cs}")
    if slopes is not None:
        if len(slopes) != 2:
            raise ValueError("slopes must be (alpha, beta)")
        rainfarm.check_nd(shape[2])
    if library is not None and (not isinstance(library, AnalogLibrary) or tuple(library.plane_shape) != shape[2:]):
        raise ValueError(f"library: expected an AnalogLibrary of planes {shape[2:]}")
    if query_groups is not None and (library is None or len(query_groups) != shape[0]):
        raise ValueError(f"query_groups: {shape[0]} groups and a library expected")
    if cascade is not None and not isinstance(cascade, CascadeModel):
        raise ValueError("cascade: expected a cascade.CascadeModel")
    cascade_patch = whole_number(cascade_patch, 1, MAX_PLANE, "cascade_patch")
    m = whole_number(n_members, 1, max_members, "n_members")
    seed = whole_number(seed, 0, (1 << 62), "seed")
    require_gpu()
    reals = device_f32(reals_precip, "reals_precip")
    reals_host = reals.cpu()                                                 # the GAN's daily sums are taken on the host, as crps_for_days does
    makers = {"gan": lambda d: gan_ensemble(gen, reals_host[d], m, seed=seed + d)}
    if slopes is not None:
        alpha, beta = float(slopes[0]), float(slopes[1])
        makers["rainfarm"] = lambda d: rainfarm.downscale_device(reals[d].sum(0), alpha, beta, n_members=m, seed=seed, first_member=d * m)
    if library is not None:
        groups = None if query_groups is None else np.asarray(query_groups)
        makers["analog"] = lambda d: library.generate(reals[d:d + 1].sum(1), m, k=k, seed=seed, weights=analog_weights, first_query=d,
                                                      query_groups=None if groups is None else groups[d:d + 1])[0]
    if cascade is not None:
        makers["cascade"] = lambda d: cascade.generate(reals[d:d + 1].sum(1), m, seed=seed, first_query=d, patch=cascade_patch)[0]
    return Roster(reals, climatology, m, makers)
