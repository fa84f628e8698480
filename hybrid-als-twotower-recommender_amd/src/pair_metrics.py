"""Spark's RegressionMetrics from the device sums of a pair list
(_hrec.PAIR_SUMS: hrec_als_pair_metrics / hrec_tt_pair_metrics), shared by
ALSModel.regression_metrics and TwoTowerModel.regression_metrics."""
import numpy as np

METRIC_NAMES = ("rmse", "mse", "mae", "r2", "var")


def regression_metrics(s, drop_nan=True):
    """{"rmse", "mse", "mae", "r2", "var", "count", "dropped"} from s, the
    {name: float} of _hrec.PAIR_SUMS (unweighted, not through the origin),
    over the n rows kept: mse = sum e^2 / n, mae = sum |e| / n, r2 = 1 - sum
    e^2 / sum (y - ybar)^2 and var = sum (p - ybar)^2 / n (ybar the label
    mean). drop_nan leaves rows with a NaN prediction out and counts them in
    "dropped"; otherwise they are kept, and one such row makes every metric
    NaN. No row kept: NaN metrics, count 0."""
    n_ok, n_nan = int(s["n_ok"]), int(s["n_nan"])
    nan = float("nan")
    res = {name: nan for name in METRIC_NAMES}
    if not drop_nan:
        res.update(count=n_ok + n_nan, dropped=0)
        if n_nan:
            return res
    else:
        res.update(count=n_ok, dropped=n_nan)
    if n_ok == 0:
        return res
    n = float(n_ok)
    ybar = s["sum_y"] / n
    ss_tot = s["sum_y2"] - s["sum_y"] * ybar                        # sum (y - ybar)^2
    ss_reg = s["sum_p2"] - 2.0 * ybar * s["sum_p"] + n * ybar * ybar  # sum (p - ybar)^2
    mse = s["sum_e2"] / n
    with np.errstate(all="ignore"):  # constant labels: ss_tot is 0 and r2 is -inf or NaN, as in Spark
        r2 = float(1.0 - np.float64(s["sum_e2"]) / np.float64(ss_tot))
    res.update(mse=mse, rmse=float(np.sqrt(mse)), mae=s["sum_abs_e"] / n, var=ss_reg / n, r2=r2)
    return res
