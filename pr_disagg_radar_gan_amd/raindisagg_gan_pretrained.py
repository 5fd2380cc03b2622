"""Drop-in for the reference's ``raindisagg_gan_pretrained.py`` (the public inference API) on the
MI355X-native engine:

    from pr_disagg_radar_gan_amd.raindisagg_gan_pretrained import generate_scenarios, plot_scenarios

Same names, argument meaning, return types and module globals (``norm_scale``,
``generator_file``, ``latent_dim``, ``gen``).  Differences, on purpose: the generator file is
loaded on first use instead of at import (the reference loads at import, :43), a ``.npz`` weight
file is accepted beside Keras ``.h5``, and a missing file raises ``FileNotFoundError`` naming it.
"""
import numpy as np

from . import models
from . import weights as W

norm_scale = W.NORM_SCALE          # reference :13
generator_file = 'trained_models/gen_20090101-20161231-tp_thresh_daily5_n_thresh20_ndomain16_stride16_0020.h5'   # :14
latent_dim = W.LATENT_DIM          # reference :47 derives it from the loaded model's first input


class _LazyGenerator:
    """Stands in for the module-level ``gen`` of the reference (:43): resolves ``generator_file`` on
    first attribute access."""

    def __init__(self):
        object.__setattr__(self, "_model", None)

    def _resolve(self):
        if self._model is None:
            object.__setattr__(self, "_model", models.load_generator(generator_file))
        return self._model

    def __getattr__(self, name):
        return getattr(self._resolve(), name)


gen = _LazyGenerator()


def set_generator(model_or_path):
    """Use another generator (a ``models.Generator`` or a weight file path) for generate_scenarios."""
    global gen, generator_file
    if isinstance(model_or_path, str):
        generator_file = model_or_path
        gen = models.load_generator(model_or_path)
    else:
        gen = model_or_path
    return gen


def generate_scenarios(cond, n_scenarios):
    """reference :52-65.  cond: ndarray (ndomain, ndomain, 1), daily sum in mm/day (un-normalised).
    Returns ndarray (n_scenarios, 24, ndomain, ndomain) in mm/h; every scenario sums to ``cond`` over
    the 24 hours.  Uses the global numpy RNG for the latent noise, like the reference (:56)."""
    # the generator takes normalized daily sums, so we have to divide by norm_scale
    cond = np.asarray(cond) / norm_scale
    latent = np.random.normal(size=(n_scenarios, latent_dim))
    cond_batch = np.repeat(cond[np.newaxis], repeats=n_scenarios, axis=0)
    generated = gen.predict([latent, cond_batch])
    generated = generated.squeeze()          # also drops the batch axis for n_scenarios == 1, as the reference does
    return generated * cond.squeeze() * norm_scale


def _daily_map(daily):
    """daily as an ndarray, without the trailing axis of 1 that ``cond`` has"""
    daily = np.asarray(daily)
    return daily[..., 0] if daily.ndim >= 3 and daily.shape[-1] == 1 else daily


def generate_scenarios_field(daily, n_scenarios, overlap=4, latent_mode="shared"):
    """generate_scenarios for a whole daily map instead of one tile (field.disaggregate on the module's ``gen`` and
    ``norm_scale``).  daily: ndarray (ny, nx) or (n_days, ny, nx), daily sums in mm/day, ny, nx >= ndomain; a trailing axis of 1, as
    ``cond`` has it, is accepted.  Returns float64 ndarray (n_scenarios, [n_days,] 24, ny, nx) in mm/h, squeezed as
    generate_scenarios squeezes; every pixel's 24 values sum to its daily value, NaN pixels give NaN.  Tiles overlap by ``overlap``
    pixels and are blended; the latent noise comes from the global numpy RNG, one vector per (scenario, day) shared by all tiles
    (``latent_mode="shared"``) or one per tile (``"independent"``).  On an (ndomain, ndomain) field with overlap 0 this is
    generate_scenarios."""
    from . import field
    daily = _daily_map(daily)
    out, _ = field.disaggregate(gen, daily, n_scenarios, overlap=overlap, latent_mode=latent_mode, norm_scale=norm_scale)
    return out.cpu().numpy().astype(np.float64).squeeze()


def scenario_products_field(daily, n_scenarios, windows=(1, 3, 6, 12, 24), probs=(0.1, 0.5, 0.9, 0.99), thresholds=None, overlap=4,
                            latent_mode="shared"):
    """Per-pixel statistics of the k-hour peaks across n_scenarios scenarios of a whole daily map (field_products.ensemble_products
    on the module's ``gen`` and ``norm_scale``), numpy in, numpy out.  daily as generate_scenarios_field takes it.  Returns a
    field_products.FieldProducts of ndarrays: quantiles ([n_days,] K, Q, ny, nx), mean ([n_days,] K, ny, nx) and exceedance
    ([n_days,] K, T, ny, nx), or None without thresholds, float32 in mm per window; peak_hour (n_scenarios, [n_days,] ny, nx) uint8,
    the hour at which each scenario's windows[0]-hour peak begins (255 at a NaN pixel).  thresholds: None, a sequence in mm (the
    same for every window) or a (K, T) array.  The hourly scenarios themselves are never held."""
    from . import field_products
    daily = _daily_map(daily)
    r = field_products.ensemble_products(gen, daily, n_scenarios, windows=windows, probs=probs, thresholds=thresholds, overlap=overlap,
                                         latent_mode=latent_mode, norm_scale=norm_scale)
    host = lambda t: None if t is None else t.cpu().numpy()
    return r._replace(quantiles=host(r.quantiles), mean=host(r.mean), exceedance=host(r.exceedance), peak_hour=host(r.peak_hour))


def verify_scenarios_field(observed, n_scenarios, thresholds, scales=(1, 3, 5, 9, 17), n_bins=11, rank_seed=0, overlap=4,
                           latent_mode="shared", scenario_chunk=16):
    """Verify n_scenarios scenarios of a whole observed day against its hours (verification.verify_field on the module's ``gen`` and
    ``norm_scale``).  observed: ndarray ([n_days,] 24, ny, nx) in mm/h; its daily sums are the condition.  thresholds: the events in
    mm/h; scales: the FSS neighbourhood widths in pixels.  Returns a verification.Verification (numpy): rank_histogram(), brier(),
    reliability_curve(t), fss().  The latent noise comes from the global numpy RNG as in generate_scenarios_field; the hourly
    scenarios are produced scenario_chunk at a time and never held together."""
    from . import verification
    return verification.verify_field(gen, np.asarray(observed), n_scenarios, thresholds, scales=scales, n_bins=n_bins,
                                     rank_seed=rank_seed, scenario_chunk=scenario_chunk, overlap=overlap, latent_mode=latent_mode,
                                     norm_scale=norm_scale)


def sal_scenarios_field(observed, n_scenarios, thresholds, connectivity=8, overlap=4, latent_mode="shared", scenario_chunk=16):
    """SAL of n_scenarios scenarios of a whole observed day against its hours (sal.sal_field on the module's ``gen`` and
    ``norm_scale``): per scenario, hour and threshold the structure, amplitude and location components of the object-based
    verification of Wernli et al. (2008).  observed: ndarray ([n_days,] 24, ny, nx) in mm/h; its daily sums are the condition.
    thresholds: the wet-pixel events in mm/h.  Returns a sal.SAL (numpy): S, A, L1, L2, L, mask_mismatch and summary().  The latent
    noise comes from the global numpy RNG as in generate_scenarios_field; the hourly scenarios are produced scenario_chunk at a time
    and never held together."""
    from . import sal
    return sal.sal_field(gen, np.asarray(observed), n_scenarios, thresholds, connectivity=connectivity, scenario_chunk=scenario_chunk,
                         overlap=overlap, latent_mode=latent_mode, norm_scale=norm_scale)


def intensity_scale_scenarios_field(observed, n_scenarios, thresholds, levels=None, overlap=4, latent_mode="shared", scenario_chunk=16):
    """The intensity-scale skill of n_scenarios scenarios of a whole observed day against its hours
    (intensity_scale.intensity_scale_field on the module's ``gen`` and ``norm_scale``): per threshold the binary error split by Haar
    wavelets into spatial scales of 1, 2, 4 ... 2^levels pixels (Casati et al. 2004).  observed: ndarray ([n_days,] 24, ny, nx) in
    mm/h; its daily sums are the condition.  thresholds: the events in mm/h; levels: the tile is 2^levels pixels wide, by default the
    largest that fits.  Returns an intensity_scale.IntensityScale (numpy): mse(), skill(), energy(), contingency(), summary().  The
    latent noise comes from the global numpy RNG as in generate_scenarios_field; the hourly scenarios are produced scenario_chunk at
    a time and never held together."""
    from . import intensity_scale
    return intensity_scale.intensity_scale_field(gen, np.asarray(observed), n_scenarios, thresholds, levels=levels,
                                                 scenario_chunk=scenario_chunk, overlap=overlap, latent_mode=latent_mode,
                                                 norm_scale=norm_scale)


def distance_scenarios_field(observed, n_scenarios, thresholds, cutoff_px=None, zhu_lambda=0.5, overlap=4, latent_mode="shared",
                             scenario_chunk=16):
    """The distance measures of n_scenarios scenarios of a whole observed day against its hours (distmap.distmap_field on the
    module's ``gen`` and ``norm_scale``): per scenario, hour and threshold how far the scenario's rain is from the observed rain, in
    pixels -- Hausdorff distance, mean error distances, Baddeley's Delta, Zhu's measure and the critical success index.  observed:
    ndarray ([n_days,] 24, ny, nx) in mm/h, ny, nx <= 2048; its daily sums are the condition.  thresholds: the events in mm/h;
    cutoff_px: Baddeley's cutoff in pixels, by default the plane's diagonal.  Returns a distmap.DistanceMeasures (numpy) with
    summary().  The latent noise comes from the global numpy RNG as in generate_scenarios_field; the hourly scenarios are produced
    scenario_chunk at a time and never held together."""
    from . import distmap
    return distmap.distmap_field(gen, np.asarray(observed), n_scenarios, thresholds, cutoff_px=cutoff_px, zhu_lambda=zhu_lambda,
                                 scenario_chunk=scenario_chunk, overlap=overlap, latent_mode=latent_mode, norm_scale=norm_scale)


def temporal_structure_field(daily, n_scenarios, thresholds, max_lag=6, overlap=4, latent_mode="shared", scenario_chunk=16):
    """The temporal structure of n_scenarios scenarios of a whole daily map (temporal.temporal_structure_field on the module's
    ``gen`` and ``norm_scale``): wet-spell and dry-spell lengths, wet hours per day, wet/dry transitions by hour, lag correlations.
    daily as generate_scenarios_field takes it; thresholds: the wet-hour events in mm/h.  Returns a temporal.TemporalStats (numpy);
    temporal.compare sets it against the same statistics of observed days.  The latent noise comes from the global numpy RNG as in
    generate_scenarios_field; the hourly scenarios are produced scenario_chunk at a time and never held together."""
    from . import temporal
    daily = _daily_map(daily)
    return temporal.temporal_structure_field(gen, daily, n_scenarios, thresholds, max_lag=max_lag, scenario_chunk=scenario_chunk,
                                             overlap=overlap, latent_mode=latent_mode, norm_scale=norm_scale)


def cell_structure_field(daily, n_scenarios, thresholds, connectivity=8, overlap=4, latent_mode="shared", scenario_chunk=16):
    """The rain cells of n_scenarios scenarios of a whole daily map (cells.cell_structure_field on the module's ``gen`` and
    ``norm_scale``): how many connected wet areas an hour has, how large they are, how much water they carry, by hour of day.
    daily as generate_scenarios_field takes it; thresholds: the wet-pixel events in mm/h.  Returns a cells.CellStats (numpy);
    cells.compare sets it against the same statistics of observed days.  The latent noise comes from the global numpy RNG as in
    generate_scenarios_field; the hourly scenarios are produced scenario_chunk at a time and never held together."""
    from . import cells
    daily = _daily_map(daily)
    return cells.cell_structure_field(gen, daily, n_scenarios, thresholds, connectivity=connectivity, scenario_chunk=scenario_chunk,
                                      overlap=overlap, latent_mode=latent_mode, norm_scale=norm_scale)


def storm_structure_field(daily, n_scenarios, thresholds, connectivity=8, reach=1, overlap=4, latent_mode="shared", scenario_chunk=16):
    """The storms of n_scenarios scenarios of a whole daily map (storms.storm_structure_field on the module's ``gen`` and
    ``norm_scale``): the wet volumes connected through the day's hours -- how long a rain system lives, when it starts, how much of
    the day's water falls in long-lived systems.  daily as generate_scenarios_field takes it; thresholds: the wet-pixel events in
    mm/h; reach: the pixels rain may move per hour and stay the same storm.  Returns a storms.StormStats (numpy); storms.compare
    sets it against the same statistics of observed days.  The latent noise comes from the global numpy RNG as in
    generate_scenarios_field; the hourly scenarios are produced scenario_chunk at a time and never held together."""
    from . import storms
    daily = _daily_map(daily)
    return storms.storm_structure_field(gen, daily, n_scenarios, thresholds, connectivity=connectivity, reach=reach,
                                        scenario_chunk=scenario_chunk, overlap=overlap, latent_mode=latent_mode, norm_scale=norm_scale)


def areal_extremes_field(daily, n_scenarios, windows=(1, 3, 6, 12, 24), widths=(1, 5, 15, 31), levels=None, overlap=4, latent_mode="shared",
                         scenario_chunk=16):
    """The areal extremes of n_scenarios scenarios of a whole daily map (areal.areal_extremes_field on the module's ``gen`` and
    ``norm_scale``): for every scenario the largest accumulation over any k consecutive hours and any w x w box of pixels -- the
    depth-area-duration table and the storm-centred areal reduction factor, which say whether the generator's peaks are too
    speckled or too smooth for a catchment.  daily as generate_scenarios_field takes it; windows: the durations in hours; widths:
    the box widths in pixels; levels: areal-mean depths in mm whose exceedance is counted (None: areal.DEFAULT_LEVELS).  Returns an
    areal.ArealStats (numpy); areal.compare sets it against the same statistics of observed days.  The latent noise comes from the
    global numpy RNG as in generate_scenarios_field; the hourly scenarios are produced scenario_chunk at a time and never held
    together."""
    from . import areal
    daily = _daily_map(daily)
    return areal.areal_extremes_field(gen, daily, n_scenarios, windows, widths, areal.DEFAULT_LEVELS if levels is None else levels,
                                      scenario_chunk=scenario_chunk, overlap=overlap, latent_mode=latent_mode, norm_scale=norm_scale)


def scaling_scenarios_field(daily, n_scenarios, space_levels=None, overlap=4, latent_mode="shared", scenario_chunk=16):
    """The scaling structure of n_scenarios scenarios of a whole daily map (scaling.scaling_structure_field on the module's ``gen``
    and ``norm_scale``): the moments, wet fraction and histogram of the rain summed over dyadic boxes of 1 .. 2^space_levels pixels a
    side and aligned windows of 1, 2, 4, 8, 24 hours -- whether the generator's fields scale as radar fields do, or are too
    intermittent at one hour or too smooth at a few pixels.  daily as generate_scenarios_field takes it; space_levels: 0 .. 6 (None:
    the largest the map admits).  Returns a scaling.ScalingStats (numpy); scaling.compare sets it against the same statistics of
    observed days.  The latent noise comes from the global numpy RNG as in generate_scenarios_field; the hourly scenarios are produced
    scenario_chunk at a time and never held together."""
    from . import scaling
    daily = _daily_map(daily)
    return scaling.scaling_structure_field(gen, daily, n_scenarios, space_levels, scenario_chunk=scenario_chunk, overlap=overlap,
                                           latent_mode=latent_mode, norm_scale=norm_scale)


def catchment_rainfall_field(daily, n_scenarios, cmap, windows=(1, 3, 6, 12, 24), levels=None, return_series=False, overlap=4,
                             latent_mode="shared", scenario_chunk=16):
    """The catchment rainfall of n_scenarios scenarios of a whole daily map (catchments.catchment_rainfall_field on the module's
    ``gen`` and ``norm_scale``): for every scenario and every basin of the catchments.CatchmentMap ``cmap`` the largest areal
    rainfall over any k consecutive hours and the hour it starts -- what a rainfall-runoff model of the basin is driven by.  daily
    as generate_scenarios_field takes it; windows: the durations in hours; levels: catchment-mean depths in mm whose exceedance is
    counted (None: catchments.DEFAULT_LEVELS).  Returns a catchments.CatchmentStats (numpy), with return_series followed by the
    hyetographs (n_scenarios, [D,] C, 24) int64 on the device (catchments.series_mm: in mm/h); catchments.compare sets the
    statistics against those of observed days.  The latent noise comes from the global numpy RNG as in generate_scenarios_field;
    the hourly scenarios are produced scenario_chunk at a time and never held together."""
    from . import catchments
    daily = _daily_map(daily)
    return catchments.catchment_rainfall_field(gen, daily, n_scenarios, cmap, windows, catchments.DEFAULT_LEVELS if levels is None else levels,
                                               return_series=return_series, scenario_chunk=scenario_chunk, overlap=overlap,
                                               latent_mode=latent_mode, norm_scale=norm_scale)


def extremes_field(daily, n_scenarios, block, n_blocks_per_member, windows=(1, 3, 6, 12, 24), min_days=1, return_sorted=False, overlap=4,
                   latent_mode="shared", scenario_chunk=16):
    """The extremes of n_scenarios scenarios of a series of daily maps (extremes.extremes_field on the module's ``gen`` and
    ``norm_scale``): for every scenario, pixel and duration the largest accumulation of each block of days -- block (D,) names the
    year or season of every day, 0 .. n_blocks_per_member - 1 -- and from those maxima the L-moment sums that give Gumbel and GEV
    return levels: the intensity-duration-frequency curves of the ensemble.  daily as generate_scenarios_field takes it; windows:
    the durations in hours, within the day.  Returns an extremes.ExtremeStats on the device, one series per scenario;
    extremes.compare sets the statistics of observed days against the band the scenarios span.  The latent noise comes from the
    global numpy RNG as in generate_scenarios_field; the hourly scenarios are produced scenario_chunk at a time and never held
    together."""
    from . import extremes
    daily = _daily_map(daily)
    return extremes.extremes_field(gen, daily, n_scenarios, block, n_blocks_per_member, windows, min_days=min_days,
                                   return_sorted=return_sorted, scenario_chunk=scenario_chunk, overlap=overlap, latent_mode=latent_mode,
                                   norm_scale=norm_scale)


def spacetime_structure_field(daily, n_scenarios, thresholds, radius=4, max_lag=1, overlap=4, latent_mode="shared", scenario_chunk=16):
    """The space-time structure of n_scenarios scenarios of a whole daily map (spacetime.spacetime_structure_field on the module's
    ``gen`` and ``norm_scale``): the wet/dry agreement of hour h at pixel p with hour h + k at pixel p + d, and the displacement
    that best maps one hour's wet mask onto the next -- does the rain travel or jump.  daily as generate_scenarios_field takes it;
    thresholds: the wet-pixel events in mm/h.  Returns a spacetime.SpaceTimeStats (numpy); spacetime.compare sets it against the
    same statistics of observed days.  The latent noise comes from the global numpy RNG as in generate_scenarios_field; the hourly
    scenarios are produced scenario_chunk at a time and never held together."""
    from . import spacetime
    daily = _daily_map(daily)
    return spacetime.spacetime_structure_field(gen, daily, n_scenarios, thresholds, radius=radius, max_lag=max_lag,
                                               scenario_chunk=scenario_chunk, overlap=overlap, latent_mode=latent_mode,
                                               norm_scale=norm_scale)


def chain_scenarios_field(daily, n_scenarios, first_hour=0, last_hour=23, overlap=4, latent_mode="shared", scenario_chunk=16,
                          matching="greedy"):
    """Chain n_scenarios scenarios of a series of daily maps (n_days, ny, nx) across midnight (sequence.chain_field on the module's
    ``gen`` and ``norm_scale``): how well every member of one day continues every member of the next, the cheapest single series,
    and a matching that orders the members of every day into n_scenarios continuous series -- the greedy one, or with
    matching="optimal" the one of least total seam cost per boundary (sequence.optimal_matching).  Returns a sequence.ChainResult
    (numpy): ``order[d][s]`` is the member of day d in series s, and sequence.reorder applies it to the hourly ensemble that
    generate_scenarios_field returns for the same numpy RNG state; sequence.compare sets the seams against observed ones.  The
    latent noise comes from the global numpy RNG as in generate_scenarios_field; the hourly scenarios are produced scenario_chunk
    at a time and never held together."""
    from . import sequence
    sequence.check_matching(matching)
    daily = _daily_map(daily)
    return sequence.chain_field(gen, daily, n_scenarios, scenario_chunk=scenario_chunk, first_hour=first_hour, last_hour=last_hour,
                                overlap=overlap, latent_mode=latent_mode, norm_scale=norm_scale, matching=matching)


def reduce_scenarios_field(daily, n_scenarios, k, pool=1, return_hourly=False, overlap=4, latent_mode="shared", scenario_chunk=16):
    """Reduce n_scenarios scenarios of a whole daily map to k representative ones (reduction.reduce_field on the module's ``gen``
    and ``norm_scale``): fast forward selection under the L1 distance of the hourly fields, pooled over pool x pool pixels, so that
    the weighted picks stay as close to the whole ensemble as k members can.  daily as generate_scenarios_field takes it.  Returns
    a reduction.Reduction (numpy): ``chosen`` (k,) the picked scenarios in order, ``weights`` their probabilities, ``assign`` the
    pick every scenario goes to, ``mean_distance_mm`` the curve on which k is chosen, ``latent`` the latent vectors that make the
    picks again, and with return_hourly ``hourly`` (k, [D,] 24, ny, nx), the picks themselves on the device.  The latent noise comes
    from the global numpy RNG as in generate_scenarios_field; the hourly scenarios are produced scenario_chunk at a time and never
    held together."""
    from . import reduction
    daily = _daily_map(daily)
    return reduction.reduce_field(gen, daily, n_scenarios, k, pool=pool, return_hourly=return_hourly, scenario_chunk=scenario_chunk,
                                  overlap=overlap, latent_mode=latent_mode, norm_scale=norm_scale)


def plot_scenarios(scenarios):
    """reference :68-90: one row per scenario, 24 hourly panels, LogNorm(0.01, 50), gist_earth_r.
    Keeps the reference's indexing ``scenarios[iplot, jplot - 1]`` (the column labelled 00:00 shows
    hour index -1, i.e. the last hour) so figures are identical to the reference's."""
    from matplotlib import pyplot as plt
    from matplotlib.colors import LogNorm

    scenarios = np.asarray(scenarios)
    nrows = len(scenarios)
    fig, axes = plt.subplots(nrows, 24, figsize=(24, nrows), squeeze=False)
    norm = LogNorm(vmin=0.01, vmax=50)
    image = None
    for (irow, hour), ax in np.ndenumerate(axes):
        image = ax.imshow(scenarios[irow, hour - 1], cmap=plt.cm.gist_earth_r, norm=norm)
        ax.set_axis_off()
        if irow == 0:
            ax.annotate(f'{hour:02d}:00', xy=(0.5, 1), xytext=(0, 5), xycoords='axes fraction',
                        textcoords='offset points', size='large', ha='center', va='baseline')
    fig.subplots_adjust(right=0.93)
    colorbar = fig.colorbar(image, cax=fig.add_axes([0.93, 0.15, 0.007, 0.7]))
    colorbar.set_label('fraction of daily precipitation', fontsize=16)
    colorbar.ax.tick_params(labelsize=16)
    return fig
