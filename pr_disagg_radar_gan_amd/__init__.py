"""MI355X-native (gfx950) cWGAN-GP hot path of RainDisaggGAN (sipposip/pr-disagg-radar-gan).

Host-side mirror of the reference's Python surface over hand-written HIP kernels:
  * ``raindisagg_gan_pretrained`` -- generate_scenarios / plot_scenarios (reference file of the same name)
  * ``gan_train_cwgangp_pixelnorm`` -- create_generator / create_discriminator / train (idem)
  * ``engine.Engine`` -- thin object over the C ABI of include/rdgan.h
  * evaluation, imported as submodules like the rest: ``ensemble``, ``spectral``, ``rainfarm``, ``crps_experiment``,
    ``distribution``
  * ``field`` -- disaggregate: whole daily fields through the generator, overlapping tiles blended on the device
  * ``field_products`` -- k-hour peaks of hourly maps and statistics across an ensemble's members, the hourly ensemble never held
  * ``verification`` -- rank histogram, Brier score with reliability table and fractions skill score of field ensembles against the
    observed hours, accumulated over groups of scenarios
  * ``spacetime`` -- displaced wet/dry agreement of hour pairs and the shift that best maps one hour's wet mask onto the next
  * ``storms`` -- wet volumes connected through the day's hours: how long a rain system lives, when it starts, what it carries
  * ``areal`` -- depth-area-duration: the largest k-hour accumulation over any w x w box per day, and the areal reduction factor
  * ``catchments`` -- catchment rainfall: the hyetograph of every basin of a map and its largest k-hour accumulation per day
  * ``analog`` -- the analog baseline (method of fragments): the k nearest library days of a daily condition, their scaled fractions
  * ``multivariate`` -- energy and variogram score of ensembles of whole hourly days; their experiment over the roster of competing methods
  * ``multivariate_ranks`` -- multivariate rank histograms of such ensembles: average-rank, band-depth and minimum-spanning-tree
    pre-ranks of the observed day, the observation's rank and the reliability index
  * ``scaling`` -- box moments over space and time: wet fraction, moments and histograms of the rain summed over dyadic boxes and
    aligned windows, their scaling exponents and the box-counting dimension
  * ``cascade`` -- the random-cascade baseline: splits of wet boxes calibrated on hourly data, applied to daily sums 24 h -> 1 h
  * ``sequence`` -- chaining scenarios across midnight: seam costs between the members of neighbouring days, the cheapest single
    series, a greedy matching into continuous series
"""
from .engine import Engine, require_gpu  # noqa: F401
from . import weights  # noqa: F401
from . import field_products  # noqa: F401
from . import verification  # noqa: F401
from . import multivariate  # noqa: F401
from . import multivariate_ranks  # noqa: F401
