"""``ELPDData``: the result object of ``loo()`` -- a ``pandas.Series`` with a report printer.

Mirrors the LOO part of the reference container (pyloo/elpd.py:100-498): same index keys,
same properties, same printed report (README.md:76-84 of the reference; the LOGO report of elpd.py:165-220), including the Pareto-k
table with bins ``(-inf, good_k], (good_k, 1], (1, inf)`` (elpd.py:300-330), the k-fold report (elpd.py:64-72, 130-163) and the
report of a Mix-IS-LOO result, which has no ``p_loo`` (elpd.py:364-374); the leave-future-out report is this package's own.  The
sub-sampling and non-factorised report variants are out of scope.
"""

from copy import copy as _copy
from copy import deepcopy as _deepcopy

import numpy as np
import pandas as pd

_REPORT = """
Computed from {n_samples} posterior samples and {n_points} observations log-likelihood matrix.

         Estimate       SE
elpd_loo   {elpd:<8.2f}    {se:<.2f}
p_loo       {p_loo:<8.2f}    {p_loo_se:<.2f}
looic      {looic:<8.2f}    {looic_se:<.2f}"""

_MIXTURE_REPORT = """
Computed from {n_samples} posterior samples and {n_points} observations log-likelihood matrix with
mixture posterior.

         Estimate       SE
elpd_loo   {elpd:<8.2f}    -"""

_WAIC_REPORT = """
Computed from {n_samples} posterior samples and {n_points} observations log-likelihood matrix.

          Estimate       SE
elpd_waic   {elpd:<8.2f}    {se:<.2f}
p_waic       {p_waic:<8.2f}        -"""

_LOGO_REPORT = """
Computed from {n_samples} posterior samples and {n_groups} groups log-likelihood matrix.

         Estimate       SE
elpd_logo   {elpd:<8.2f}    {se:<.2f}
p_logo       {p_logo:<8.2f}    {p_logo_se:<.2f}
logoic      {logoic:<8.2f}    {logoic_se:<.2f}"""

_KFOLD_REPORT = """
Computed from {n_samples} posterior samples using {K}-fold cross-validation
with {n_points} observations.{stratify_msg}

           Estimate       SE
elpd_kfold   {elpd:<8.2f}    {se:<.2f}
p_kfold       {p_kfold:<8.2f}    {p_kfold_se:<.2f}
kfoldic      {kfoldic:<8.2f}    {kfoldic_se:<.2f}
"""

_LFO_REPORT = """
Computed from {n_samples} posterior samples using {M}-step-ahead leave-future-out cross-validation
with {n_points} steps (L = {L}), {n_refits} refits at k > {thr:.2f}.

         Estimate       SE
elpd_lfo   {elpd:<8.2f}    {se:<.2f}
"""

_K_TABLE = """
------

Pareto k diagnostic values:
                         Count   Pct.
(-Inf, {gk:.2f}]   (good)      {c0:d}   {p0:.1f}%
   ({gk:.2f}, 1]   (bad)         {c1:d}    {p1:.1f}%
   (1, Inf)   (very bad)    {c2:d}    {p2:.1f}%"""

_ALL_GOOD = "\n\nAll Pareto k estimates are good (k < {gk:.1f}).\nSee help('pareto-k-diagnostic') for details."
_SOME_HIGH = (
    "\n\nSome Pareto k diagnostic values are high (k > {gk:.1f}), indicating that the importance"
    " sampling approximation is unreliable. Consider using moment matching or exact LOO for more"
    " accurate estimates. Use pointwise=True to see detailed diagnostics."
)
_WARNED = "\n\nThere has been a warning during the calculation. Please check the results."


def _k_values(k):
    """The Pareto k of a result as a flat float array: a DataArray, an ndarray or a device tensor (``loo_i`` and ``pareto_k`` of a
    ``*_from_matrix`` call on a CUDA tensor stay on the device)."""
    if hasattr(k, "detach"):
        k = k.detach().cpu().numpy()
    return np.asarray(getattr(k, "values", k), dtype=float).ravel()


class ELPDData(pd.Series):
    """Expected-log-pointwise-predictive-density results with a friendly ``print``."""

    _metadata = ["_method", "_K", "_stratified", "_grouped"]

    @property
    def _constructor(self):  # keep the subclass through pandas operations
        return ELPDData

    def __str__(self):
        kind = str(self.index[0]).split("_")[-1]
        if kind == "waic":
            # The reference's printer accepts the kind (elpd.py:125) but then reads loo-only keys; this
            # report follows its standard layout with the WAIC rows.
            text = _WAIC_REPORT.format(n_samples=self.n_samples, n_points=self.n_data_points, elpd=self["elpd_waic"],
                                       se=self["se"], p_waic=self["p_waic"])
            return text + (_WARNED if self.warning else "")
        if kind == "logo":
            return self._logo_report()
        if kind == "kfold":
            # elpd.py:130-163 (kfoldic is printed as -2 elpd_kfold whatever the scale, as the reference does)
            text = _KFOLD_REPORT.format(n_samples=self.n_samples, K=self.K, n_points=self.n_data_points, elpd=self["elpd_kfold"],
                                        se=self["se"], p_kfold=self["p_kfold"], p_kfold_se=self["p_kfold_se"],
                                        kfoldic=-2 * self["elpd_kfold"], kfoldic_se=2 * self["se"],
                                        stratify_msg=" Using stratified k-fold cross-validation" if self.stratified else "")
            return text + (_WARNED if self.warning else "")
        if kind == "lfo":
            return self._lfo_report()
        if kind != "loo":
            raise ValueError("Invalid ELPDData object")
        tail = ""
        if "pareto_k" in self and self.get("good_k", None) is not None:
            gk = self["good_k"]
            kv = _k_values(self["pareto_k"])
            counts = np.histogram(kv, bins=np.asarray([-np.inf, gk, 1, np.inf]))[0]
            if counts[1] == 0 and counts[2] == 0:
                tail = _ALL_GOOD.format(gk=gk)
            else:
                pct = counts / counts.sum() * 100
                tail = _K_TABLE.format(gk=gk, c0=int(counts[0]), c1=int(counts[1]), c2=int(counts[2]),
                                       p0=pct[0], p1=pct[1], p2=pct[2])
        elif self.method == "psis":
            tail = (_SOME_HIGH if self.warning else _ALL_GOOD).format(gk=0.7)
        if "p_loo" not in self and "looic" not in self and "se" in self:  # a Mix-IS-LOO result (elpd.py:364-374): its index, whole
            text = _MIXTURE_REPORT.format(n_samples=self.n_samples, n_points=self.n_data_points, elpd=self["elpd_loo"])
        else:
            text = _REPORT.format(
                n_samples=self.n_samples, n_points=self.n_data_points, elpd=self["elpd_loo"], se=self["se"],
                p_loo=self["p_loo"], p_loo_se=self["p_loo_se"], looic=self["looic"], looic_se=self["looic_se"],
            )
        if self.warning:
            text += _WARNED
        return text + tail

    def _logo_report(self):
        """elpd.py:165-220: LOGO_BASE_FMT, the warning line, then the Pareto-k table (or the all-good line) when k is there."""
        text = _LOGO_REPORT.format(n_samples=self.n_samples, n_groups=self["n_groups"], elpd=self["elpd_logo"], se=self["se"],
                                   p_logo=self["p_logo"], p_logo_se=self.get("p_logo_se", float("nan")), logoic=self["logoic"],
                                   logoic_se=self["logoic_se"])
        if self.warning:
            text += _WARNED
        if "pareto_k" in self and self.get("good_k", None) is not None:
            gk = self["good_k"]
            kv = _k_values(self["pareto_k"])
            counts = np.histogram(kv, bins=np.asarray([-np.inf, gk, 1, np.inf]))[0]
            if counts[1] == 0 and counts[2] == 0:
                text += _ALL_GOOD.format(gk=gk)
            else:
                pct = counts / counts.sum() * 100
                text += _K_TABLE.format(gk=gk, c0=int(counts[0]), c1=int(counts[1]), c2=int(counts[2]), p0=pct[0], p1=pct[1], p2=pct[2])
        return text

    def _lfo_report(self):
        """Leave-future-out CV (loo_lfo.py), in the style of the k-fold report: the header, the warning line, then the Pareto k of
        the steps against the refit threshold when k is there (steps without one -- NaN -- are left out)."""
        text = _LFO_REPORT.format(n_samples=self.n_samples, M=self["M"], n_points=self.n_data_points, L=self["L"],
                                  n_refits=self["n_refits"], thr=self["k_threshold"], elpd=self["elpd_lfo"], se=self["se"])
        if self.warning:
            text += _WARNED
        if "pareto_k" in self:
            gk = self["k_threshold"]
            kv = _k_values(self["pareto_k"])
            kv = kv[~np.isnan(kv)]
            if np.isfinite(gk) and gk < 1 and kv.size:
                counts = np.histogram(kv, bins=np.asarray([-np.inf, gk, 1, np.inf]))[0]
                if counts[1] == 0 and counts[2] == 0:
                    text += _ALL_GOOD.format(gk=gk)
                else:
                    pct = counts / counts.sum() * 100
                    text += _K_TABLE.format(gk=gk, c0=int(counts[0]), c1=int(counts[1]), c2=int(counts[2]), p0=pct[0], p1=pct[1], p2=pct[2])
        return text

    def __repr__(self):
        return self.__str__()

    def copy(self, deep=True):
        out = pd.Series.copy(self)
        for key in out.keys():
            out[key] = _deepcopy(out[key]) if deep else _copy(out[key])
        return ELPDData(out)

    @property
    def n_samples(self):
        return self["n_samples"]

    @property
    def n_data_points(self):
        return self["n_data_points"]

    @property
    def warning(self):
        return self["warning"]

    @property
    def method(self):
        return getattr(self, "_method", "psis")

    @method.setter
    def method(self, value):
        object.__setattr__(self, "_method", value)

    @property
    def K(self):
        """Number of folds of a k-fold result."""
        return getattr(self, "_K", None)

    @K.setter
    def K(self, value):
        object.__setattr__(self, "_K", value)

    @property
    def stratified(self):
        return getattr(self, "_stratified", False)

    @stratified.setter
    def stratified(self, value):
        object.__setattr__(self, "_stratified", value)

    @property
    def grouped(self):
        return getattr(self, "_grouped", False)

    @grouped.setter
    def grouped(self, value):
        object.__setattr__(self, "_grouped", value)
