"""npbnn_amd — MI355X-native backend for npBNN's MCMC hot path.

Flat namespace like the reference package (``import npbnn_amd as bn``): ``bn.npBNN``, ``bn.MCMC``,
``bn.MC3``, ``bn.ActFun``, ``bn.run_mcmc``, ``bn.RunPredict`` ...  The per-proposal forward pass +
likelihood of the Metropolis-Hastings loop runs in hand-written HIP kernels (gfx950) behind the C ABI
declared in ``include/npbnn_hip.h``; host code is Python + ctypes.  There is no CPU fallback: without
the built library and an MI355X the device-backed calls raise ``BackendUnavailable``.
"""
__version__ = "0.1.0"

from ._capi import BackendUnavailable, NpbnnError  # noqa: F401
from .backend import HipContext, pack_weights  # noqa: F401
from .proposals import *  # noqa: F401,F403
from .proposals import init_weight_prm  # noqa: F401
from .layers import (ActFun, MatrixMultiplication, MatrixMultiplicationD, RegressTransform,  # noqa: F401
                     RegressTransformError, RunHiddenLayer, RunPredict, RunPredictInd, SoftMax, SoftPlus,
                     create_mask, leaky_relu_f, relu_f, swish_f, tanh_f)
from .likelihoods import (CalcAccuracy, CalcAccuracyRegression, CalcLabelAccuracy,  # noqa: F401
                          CalcLabelAccuracyRegression, CalcLabelFreq, SkipAccuracy, SkipAccuracyVec,
                          calc_likelihood, calc_likelihood_regression, calc_likelihood_regression_error, gamma_acc,
                          gamma_likelihood,
                          negbin2d_acc, negbin_acc, negbin_acc_base10, negbin_likelihood, negbin_likelihood2d,
                          negbin_likelihood_base10, poi_acc, poi_likelihood)
from .model import data_transform_obj, npBNN  # noqa: F401
from .sampler import MCMC, predict  # noqa: F401
from .driver import run_mcmc  # noqa: F401
from .files import (DetachedMatrix, SaveObject, attach_data, get_data, load_obj, randomize_data,  # noqa: F401
                    turn_labels_to_numeric)
from .logger import init_output_files, postLogger  # noqa: F401
from .mc3 import MC3  # noqa: F401
from .posterior import (feature_importance, get_posterior_cat_prob, get_posterior_est, predictBNN,  # noqa: F401
                        sample_from_categorical)
from .support import (CalcAccAboveThreshold, CalcConfusionMatrix, CalcFP, CalcFP_BF, CalcTP, CalcTP_BF,  # noqa: F401
                      get_accuracy_threshold, get_posterior_threshold, turn_low_pp_instances_to_nan)
from .pdp import get_feature_summary, get_pdp, make_pdp_features, pdp  # noqa: F401
from .ale import ale, get_ale, make_ale_edges  # noqa: F401
from .saliency import get_saliency, saliency  # noqa: F401
from .shapley import get_shapley, shapley  # noqa: F401
from .gradient import log_posterior_grad, loglik_grad, map_estimate  # noqa: F401
from .hpd import calcHPD, get_posterior_hpd, posterior_hpd  # noqa: F401
from .lppd import get_posterior_lppd, posterior_lppd  # noqa: F401
from .loo import get_posterior_loo, loo_compare, posterior_loo  # noqa: F401
from .uncertainty import get_posterior_uncertainty, posterior_uncertainty  # noqa: F401
from .calibration import get_posterior_calibration, posterior_calibration  # noqa: F401
from .convergence import get_posterior_convergence, posterior_convergence  # noqa: F401
from .predictive import get_posterior_predictive, posterior_predictive  # noqa: F401
from . import comm  # noqa: F401

BNN = npBNN                       # BASELINE.json's wording
