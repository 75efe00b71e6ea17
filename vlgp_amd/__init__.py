"""vlgp_amd -- MI355X-native variational-EM engine for vLGP: a drop-in for the
``vlgp.fit`` hot path of catniplab/vlgp (hand-written HIP kernels behind a C ABI,
NumPy host)."""
from .api import fit, forecast, refit_joint, sample_posterior, transform  # noqa: F401
from .util import load, save  # noqa: F401
from .engine import (DeviceTrials, Engine, VlgpError, constrain_latent, constrain_loading,  # noqa: F401
                     estep, hstep, infer, make_cholesky, mstep, update_v, update_w, vem)
from .preprocess import get_config, get_params  # noqa: F401
from . import evaluation  # noqa: F401,E402
from .evaluation import impute  # noqa: F401,E402
from . import model_selection  # noqa: F401,E402
from .model_selection import cross_validate  # noqa: F401,E402

__all__ = ["fit", "transform", "forecast", "refit_joint", "Engine", "DeviceTrials", "VlgpError", "evaluation", "model_selection", "cross_validate", "impute"]
