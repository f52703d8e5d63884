"""``scarlet.lite`` on the GPU: same names as the reference's lite package
(scarlet/lite/__init__.py), the fitting loop of ``LiteBlend.fit`` on the device."""

from .catalog import measure_blends, plan_measure_blends  # noqa: F401
from .fitting import fit_blends  # noqa: F401
from .initialization import (  # noqa: F401
    get_min_psf,
    init_adaprox_component,
    init_all_sources_main,
    init_all_sources_wavelets,
    init_blends,
    init_blends_main,
    init_fista_component,
    init_main_parameters,
    init_monotonic_morph,
    init_wavelet_source,
    multifit_seds,
    parameterize_sources,
    plan_init_blends,
    plan_init_blends_main,
    WaveletInitParameters,
)
from .measure import calculate_snr, weight_blends, weight_sources  # noqa: F401
from .models import (  # noqa: F401
    LiteBlend,
    LiteComponent,
    LiteFactorizedComponent,
    LiteObservation,
    LiteSource,
)
from .parameters import (  # noqa: F401
    AdaproxParameter,
    FistaParameter,
    LiteParameter,
    grow_array,
)
from .spectra import fit_spectra_blends, plan_fit_spectra_blends  # noqa: F401
from .utils import (  # noqa: F401
    bounds_to_bbox,
    get_circle_mask,
    insert_image,
    integrated_circular_gaussian,
    integrated_gaussian,
    project_morph_to_center,
)
