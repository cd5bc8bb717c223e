"""dcfm_amd — MI355X-native hot path of the divide-and-conquer Bayesian factor model.

Drop-in for the iteration loop of the reference ``divideconquer.m`` (lines
90-197: per-shard Gibbs sweep + covariance assembly), behind the C ABI in
``include/dcfm.h``; HIP kernels for gfx950 live in ``csrc/``.

Import through the repo-root helper (the directory name has hyphens)::

    import __graft_entry__ as ge; dcfm = ge.load_package()
    Sigmaout = dcfm.divideconquer(Y, g, k, BURNIN, MCMC, thin, rho)
"""
from ._abi import DcfmError, load_library, EXPORTS, LIB_PATH
from .sampler import Hyper, Sampler, rng_fill, count_nonzero_columns, STATE_FIELDS
from . import diagnostics
from .diagnostics import heldout_log_density, summarize_probes, partial_correlations, partial_correlation_edges, correlation, waic, conditional_log_density, regression_summary
from .driver import divideconquer, preprocess, preprocess_device, shard_columns, partition_standardize, initial_state, local_state, truth_factors, output_columns, unpermute_sigma, unpermute_vectors, permute_vectors, unpermute_precision, unpermute_partial, unpermute_corr, unpermute_communality
from .driver import preprocess_missing, partition_standardize_missing, observed_moments, unstandardize_imputation
from .driver import column_moments, unstandardize_prediction, unstandardize_regression

__all__ = [
    "preprocess_missing", "partition_standardize_missing", "observed_moments", "unstandardize_imputation",
    "DcfmError", "load_library", "EXPORTS", "LIB_PATH", "Hyper", "Sampler", "rng_fill",
    "STATE_FIELDS", "divideconquer", "preprocess", "partition_standardize", "initial_state",
    "local_state", "truth_factors", "output_columns", "unpermute_sigma", "count_nonzero_columns",
    "preprocess_device", "shard_columns", "diagnostics", "unpermute_vectors", "permute_vectors",
    "summarize_probes",
    "heldout_log_density", "unpermute_precision", "partial_correlations", "unpermute_partial", "partial_correlation_edges",
    "correlation", "unpermute_corr", "unpermute_communality", "waic", "conditional_log_density",
    "regression_summary", "column_moments", "unstandardize_prediction", "unstandardize_regression",
]
