"""pyloo_amd -- MI355X-native PSIS-LOO engine behind pyloo's ``loo`` / ``psislw`` /
``compute_importance_weights`` API.  The compute path is hand-written HIP (gfx950) reached
through the C ABI in ``include/pyloo_amd.h``; there is no CPU fallback."""

from .base import ISMethod, compute_importance_weights
from .compare import compare_weights, loo_compare
from .e_loo import ExpectationResult, compute_pareto_k, e_loo, k_hat
from .elpd import ELPDData
from .loo import loo, loo_from_matrix
from .loo_diagnostics import LooDiagnostics, loo_diagnostics, loo_diagnostics_from_matrix, pareto_k_table
from .loo_influence import LooInfluence, influence_table, loo_influence, loo_influence_from_matrix
from .loo_glm import glm_log_lik, glm_plpd, loo_glm, loo_glm_from_design, loo_subsample_glm
from .loo_glm_predict import LooGlmPredict, loo_glm_predict, loo_glm_predict_from_design
from .loo_glm_marginal import glm_marginal_log_lik, loo_glm_marginal, loo_glm_marginal_from_design
from .loo_approximate_posterior import loo_approximate_posterior, loo_approximate_posterior_from_matrix
from .loo_lfo import loo_lfo, loo_lfo_from_matrix
from .loo_kfold import kfold_split_grouped, kfold_split_random, kfold_split_stratified, loo_kfold, loo_kfold_from_matrix
from .loo_mixture import loo_mixture, loo_mixture_from_matrix
from .loo_group import GroupIndex, group_index, loo_group, loo_group_from_matrix
from .loo_pit import LooPitResult, loo_pit, loo_pit_from_matrix
from .loo_nonfactor import loo_nonfactor, loo_nonfactor_from_arrays, nonfactor_log_lik
from .loo_i import loo_i
from .loo_moment_match import loo_moment_match, loo_moment_match_split
from .loo_predictive_metric import loo_predictive_metric, predictive_metric_from_matrix
from .loo_score import LooScoreResult, loo_score, score_from_matrix
from .loo_subsample import importance_resample, loo_subsample, loo_subsample_from_matrix
from .psis import psislw
from .rcparams import rcParams
from .relative_eff import relative_eff, relative_eff_from_matrix
from .waic import waic, waic_from_matrix

__all__ = ["ISMethod", "ELPDData", "compare_weights", "loo_compare", "ExpectationResult", "compute_importance_weights", "compute_pareto_k", "e_loo", "k_hat", "loo", "loo_from_matrix", "GroupIndex", "group_index", "loo_group", "loo_group_from_matrix", "loo_i", "loo_moment_match", "loo_moment_match_split", "loo_nonfactor", "loo_nonfactor_from_arrays", "nonfactor_log_lik", "loo_predictive_metric", "predictive_metric_from_matrix", "loo_score", "score_from_matrix", "LooScoreResult", "loo_subsample",
           "loo_subsample_from_matrix", "importance_resample", "loo_approximate_posterior", "loo_approximate_posterior_from_matrix", "loo_kfold", "loo_kfold_from_matrix", "kfold_split_random", "kfold_split_stratified", "kfold_split_grouped", "loo_mixture", "loo_mixture_from_matrix", "loo_pit", "loo_pit_from_matrix", "LooPitResult", "loo_lfo", "loo_lfo_from_matrix", "relative_eff", "relative_eff_from_matrix", "loo_diagnostics", "loo_diagnostics_from_matrix", "pareto_k_table", "LooDiagnostics", "loo_influence", "loo_influence_from_matrix", "influence_table",
           "LooInfluence", "glm_log_lik", "glm_plpd", "loo_glm", "loo_glm_from_design", "loo_subsample_glm", "glm_marginal_log_lik",
           "loo_glm_marginal", "loo_glm_marginal_from_design", "LooGlmPredict", "loo_glm_predict", "loo_glm_predict_from_design", "psislw", "rcParams", "waic",
           "waic_from_matrix"]
__version__ = "0.1.0"
