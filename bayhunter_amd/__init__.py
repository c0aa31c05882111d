"""bayhunter_amd -- MI355X-native forward-model + likelihood engine behind BayHunter's plugin
surface.  Importing this package does not touch the GPU; the native library is
loaded when the first `Engine` is created."""
from .engine import Engine, EngineError, default_engine, pack_models  # noqa: F401
from .Models import Model, ModelMatrix  # noqa: F401
from .surf96_modsw import SurfDisp  # noqa: F401
from .surf96_ellip import SurfEllip  # noqa: F401
from .rfmini_modrf import RFminiModRF  # noqa: F401
from .Targets import (ObservedData, ModeledData, Valuation, SingleTarget, JointTarget,  # noqa: F401
                      RayleighDispersionPhase, RayleighDispersionGroup, LoveDispersionPhase,
                      LoveDispersionGroup, PReceiverFunction, SReceiverFunction, RayleighEllipticity, select_noise_laws)
from .chains import ChainBatch, MCMC_Optimizer  # noqa: F401
from .results import save_config, save_final_distribution, get_outliers, posterior_from_storage, moho_from_storage, features_from_storage, covariance_from_storage, datafits_from_storage, residuals_from_storage, diagnostics_from_storage  # noqa: F401
from .sites import SiteTargets  # noqa: F401
from .posterior import posterior_models, posterior_hist2d, posterior_moho, posterior_scalars, posterior_covariance, posterior_features, check_features, posterior_classes, check_classes  # noqa: F401

from .datafits import posterior_datafits, posterior_residuals  # noqa: F401
from .diagnostics import chain_series_stats, chain_model_stats, convergence, outlier_chains  # noqa: F401


def __getattr__(name):  # DeviceChains needs torch: imported on first use only
    if name == "DeviceChains":
        from .device_chains import DeviceChains
        return DeviceChains
    raise AttributeError(name)


__version__ = "0.1.0"
