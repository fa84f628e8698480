"""numpy restatement of hrec_tt_fold_in_users (include/hrec.h): one user's
embedding row fitted to its own history with everything else frozen, in the
arithmetic of `dtype` (np.float32: the kernel's formats, numpy's summation
orders; np.float64: the same recurrence in exact-enough arithmetic, the tests'
reference). Hyper-parameters are the f32 values the kernel receives, widened."""
import numpy as np

LN_EPS = 1e-3
BETA_1, BETA_2, EPSILON = np.float32(0.9), np.float32(0.999), np.float32(1e-7)


def random_case(d, history_lengths, n_items=40, seed=0, extra_rows=0):
    """Seeded f32 operands shaped like a trained model's: Keras-init start
    rows (uniform +-0.05), LayerNorm weights near (1, 0), item vectors of O(1)
    entries (LayerNorm outputs), ratings in [1, 5]. A dict with emb
    [len(history_lengths) + extra_rows, d], gamma, beta, item_vec [n_items, d],
    indptr (over the first len(history_lengths) rows), item_rows, ratings."""
    rng = np.random.default_rng([seed, d, len(history_lengths)])
    lens = np.asarray(history_lengths, np.int64)
    nnz = int(lens.sum())
    return {
        "emb": rng.uniform(-0.05, 0.05, (lens.size + extra_rows, d)).astype(np.float32),
        "gamma": (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32),
        "beta": (0.1 * rng.standard_normal(d)).astype(np.float32),
        "item_vec": rng.standard_normal((n_items, d)).astype(np.float32),
        "indptr": np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
        "item_rows": rng.integers(0, n_items, nnz).astype(np.int64),
        "ratings": rng.uniform(1.0, 5.0, nnz).astype(np.float32),
    }


def step_sizes(learning_rate, steps, beta_1=BETA_1, beta_2=BETA_2):
    """f32 [steps]: lr * sqrt(1 - beta_2^t) / (1 - beta_1^t) for t = 1 .. steps,
    rounded as OptimizerV2 Adam._prepare_local rounds it in f32."""
    lr, b1, b2, one = np.float32(learning_rate), np.float32(beta_1), np.float32(beta_2), np.float32(1.0)
    out = np.empty(int(steps), np.float32)
    for i in range(int(steps)):
        t = np.float32(i + 1)
        b1p = np.float32(np.power(b1, t, dtype=np.float32))
        b2p = np.float32(np.power(b2, t, dtype=np.float32))
        out[i] = np.float32(lr * np.float32(np.sqrt(np.float32(one - b2p)) / np.float32(one - b1p)))
    return out


def layer_norm(e, gamma, beta, dtype):
    """(u, xhat, rstd) of Keras LayerNormalization(epsilon=1e-3) on one row."""
    dt = np.dtype(dtype).type
    d = dt(e.size)
    mean = e.sum(dtype=dtype) / d
    t = e - mean
    var = (t * t).sum(dtype=dtype) / d
    rstd = dt(1.0) / np.sqrt(var + dt(LN_EPS))
    xh = t * rstd
    return xh * gamma + beta, xh, rstd


def loss_and_gradient(e, gamma, beta, vecs, ratings, dtype):
    """(mean squared error, its gradient with respect to e, u) for one row
    whose usable history is (vecs [n, d], ratings [n]), n >= 1."""
    dt = np.dtype(dtype).type
    n, d = dt(ratings.size), dt(e.size)
    u, xh, rstd = layer_norm(e, gamma, beta, dtype)
    err = vecs @ u - ratings
    loss = (err * err).sum(dtype=dtype) / n
    du = (dt(2.0) / n) * (err @ vecs)
    dxh = du * gamma
    g = rstd * (dxh - dxh.sum(dtype=dtype) / d - xh * ((dxh * xh).sum(dtype=dtype) / d))
    return loss, g, u


def fold_in(emb, gamma, beta, item_vec, indptr, item_rows, ratings, steps, step_lr, dtype=np.float64,
            beta_1=BETA_1, beta_2=BETA_2, epsilon=EPSILON):
    """(emb_out [n_rows, d], u_out [n_rows, d] = LN(emb_out), loss [n_rows, 2])
    in `dtype`. A row without a usable entry keeps its bits and gets NaN
    losses; steps == 0 keeps every row and gives the same loss twice."""
    dt = np.dtype(dtype).type
    emb = np.array(emb, dtype=dtype)
    gamma, beta = np.asarray(gamma, dtype), np.asarray(beta, dtype)
    item_vec = np.asarray(item_vec, dtype).reshape(-1, emb.shape[1])
    lr = np.asarray(step_lr, np.float32).astype(dtype)
    b1, b2, eps = dt(np.float32(beta_1)), dt(np.float32(beta_2)), dt(np.float32(epsilon))
    omb1, omb2 = dt(np.float32(1.0) - np.float32(beta_1)), dt(np.float32(1.0) - np.float32(beta_2))
    n_items = item_vec.shape[0]
    u_out = np.empty_like(emb)
    loss = np.full((emb.shape[0], 2), np.nan, dtype)
    for r in range(emb.shape[0]):
        rows = np.asarray(item_rows[indptr[r]: indptr[r + 1]], np.int64)
        keep = (rows >= 0) & (rows < n_items)
        vecs = item_vec[rows[keep]]
        y = np.asarray(ratings[indptr[r]: indptr[r + 1]], dtype)[keep]
        e = emb[r].copy()
        if y.size == 0:
            u_out[r] = layer_norm(e, gamma, beta, dtype)[0]
            continue
        m, v = np.zeros_like(e), np.zeros_like(e)
        for t in range(int(steps) + 1):
            cur, g, u = loss_and_gradient(e, gamma, beta, vecs, y, dtype)
            if t == 0:
                loss[r, 0] = cur
            if t == int(steps):
                break
            m = m * b1 + g * omb1
            v = v * b2 + (g * g) * omb2
            e = e - (lr[t] * m) / (np.sqrt(v) + eps)
        loss[r, 1] = cur
        emb[r], u_out[r] = e, u
    return emb, u_out, loss
