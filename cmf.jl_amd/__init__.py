"""cmf.jl_amd -- MI355X (gfx950) implementation of CMF.jl's update rules (MU, HALS, PGD, ADMM, ANLS) and its separable fit.

The directory name is not a Python identifier; import it through the shim at the
repo root:  ``import cmf_jl_amd as cmf``.
"""
from ._lib import CMFError, LIB_PATH, SYMBOLS, load as load_library  # noqa: F401
from .host import (  # noqa: F401
    EPSILON, ADMMUpdate, ANLSUpdate, AbsoluteLoss, AbsolutePenalty, AbstractCFUpdate, AlternatingOptimizer, CNMF_results, HALSUpdate, HIPADMMUpdate, HIPANLSUpdate, HIPHALSUpdate,
    HIPMultUpdate, HIPPGDUpdate, MaskedLoss, MultUpdate, NonnegConstraint, PGDUpdate, SquareLoss, SquarePenalty, UnitNormConstraint,
    compute_loss, converged, cross_validate, evaluate_convergence, evaluate_divergence, evaluate_heldout, evaluate_mse, evaluate_test, evaluate_xortho, xortho_sweep, evaluate_significance, significance_from_sums, null_shifts, recentre, SignificanceResult, holdout_mask, fit, fit_cnmf, gen_synthetic,
    init_rand, load_model, parameter_sweep, rccl_version, save_model, tensor_conv, tensor_transconv,
    EventData, EventKLUpdate, init_rand_events,
    Separable, cos_score, gen_sep_data, is_separable, permute_factors, row_normalize, separable_fit,
)

__version__ = "0.1.0"
