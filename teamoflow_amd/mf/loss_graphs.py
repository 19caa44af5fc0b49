"""Loss graphs (plug-in interface of /root/reference/src/teamoflow/mf/loss_graphs.py).

``MSELoss``, ``WMRBLoss``, ``KLDivergenceLoss``, ``LogisticLoss``, ``BPRLoss``, ``WARPLoss``, ``KOSWARPLoss``, ``SampledSoftmaxLoss``
and ``FullSoftmaxLoss`` (extensions: the reference has no logistic loss, pointwise or pairwise, no first-violator ranking loss and no
softmax, sampled or over the whole catalog - the last one reads no negative table: its partition is swept through the matrix cores,
csrc/tmf_fullsoftmax.hip) with ``LinearEmbedding`` over indicator features are recognised by
``MatrixFactorization.fit`` (same isinstance dispatch as matrix_factorization.py:152-162) and run as
fused HIP kernels; ``get_loss`` below is the generic differentiable definition used when the model is
built from other plug-ins (dense features, custom embeddings), always called by keyword like
matrix_factorization.py:165-167 does.
"""
import math
from abc import ABC, abstractmethod

import torch


class _TFMaximum(torch.autograd.Function):
    """tf.maximum semantics: the gradient goes to x where x >= y (ties included)."""

    @staticmethod
    def forward(ctx, x, y):
        ctx.save_for_backward(x >= y)
        return torch.maximum(x, y)

    @staticmethod
    def backward(ctx, g):
        (m,) = ctx.saved_tensors
        zero = torch.zeros_like(g)
        return torch.where(m, g, zero), torch.where(m, zero, g)


class LossGraph(ABC):
    """loss_graphs.py:8-28: returns the 1-D per-interaction loss vector."""

    @abstractmethod
    def get_loss(self, tf_interactions, tf_sample_predictions, tf_prediction_serial, predictions, n_items, n_samples):
        pass


class MSELoss(LossGraph):
    """loss_graphs.py:31-52: squared error on every stored interaction."""

    def get_loss(self, tf_interactions, predictions, tf_sample_predictions=None, tf_prediction_serial=None,
                 n_items=None, n_samples=None):
        idx = tf_interactions.indices
        return torch.square(tf_interactions.values - predictions[idx[:, 0], idx[:, 1]])


class WMRBLoss(LossGraph):
    """loss_graphs.py:55-88: log(1 + (n_items / n_samples) * sum_s max(1 - p_k + sp[u_k, s], 0)) for
    the positive interactions only."""

    def get_loss(self, tf_interactions, tf_sample_predictions, tf_prediction_serial, n_items, n_samples,
                 predictions=None):
        mask = tf_interactions.values > 0.0
        users = tf_interactions.indices[:, 0][mask]
        pos = tf_prediction_serial[mask]
        x = 1.0 - pos[:, None] + tf_sample_predictions[users]
        hinge = _TFMaximum.apply(x, torch.zeros_like(x))
        return torch.log(1.0 + (n_items / n_samples) * hinge.sum(dim=1))


class KLDivergenceLoss(LossGraph):
    """loss_graphs.py:91-122: 1 - CDF_{N(mu_neg - mu_pos, sqrt(var_pos + var_neg))}(0); a single scalar.
    The normal CDF is written with erf (the reference uses tensorflow-probability)."""

    def get_loss(self, tf_prediction_serial, tf_interactions, tf_sample_predictions=None, predictions=None,
                 n_items=None, n_samples=None):
        pos_mask = tf_interactions.values > 0.0
        pos, neg = tf_prediction_serial[pos_mask], tf_prediction_serial[~pos_mask]
        loc = neg.mean() - pos.mean()
        scale = torch.sqrt(pos.var(unbiased=False) + neg.var(unbiased=False))
        cdf0 = 0.5 * (1.0 + torch.erf((0.0 - loc) / (scale * 2.0 ** 0.5)))
        return 1.0 - cdf0


class LogisticLoss(LossGraph):
    """Extension (LightFM's default objective; not in the reference): the pointwise logistic loss over signed feedback.  For every
    stored interaction with score p:  y = +1 where the value is > 0, else -1 (KLDivergenceLoss's class split: a stored 0 is a
    negative),  w = |value| if ``weighted`` else 1,  loss = w log(1 + exp(-y p)),  d loss / d p = -y w sigmoid(-y p)."""

    def __init__(self, weighted=False):
        self.weighted = bool(weighted)

    def get_loss(self, tf_interactions, predictions, tf_sample_predictions=None, tf_prediction_serial=None,
                 n_items=None, n_samples=None):
        idx, values = tf_interactions.indices, tf_interactions.values
        p = predictions[idx[:, 0], idx[:, 1]]
        y = torch.where(values > 0.0, torch.ones_like(p), -torch.ones_like(p))
        w = values.abs().to(p.dtype) if self.weighted else torch.ones_like(p)
        return -w * torch.nn.functional.logsigmoid(y * p)


class BPRLoss(LossGraph):
    """Extension (Bayesian personalised ranking, LightFM's and implicit's 'bpr'; not in the reference): the pairwise logistic loss over
    the static negative table WMRBLoss samples from.  For every stored interaction k of user u with a value > 0 and score p_k, against
    the user's row sp[u, :] of sampled scores:  loss_k = mean_s -log sigmoid(p_k - sp[u, s]).  Stored values <= 0 take no part, a
    negative that coincides with one of the user's positives is not filtered (both as in WMRBLoss), and n_items / n_samples does
    not enter."""

    def get_loss(self, tf_interactions, tf_sample_predictions, tf_prediction_serial, n_items, n_samples, predictions=None):
        mask = tf_interactions.values > 0.0
        users = tf_interactions.indices[:, 0][mask]
        pos = tf_prediction_serial[mask]
        return -torch.nn.functional.logsigmoid(pos[:, None] - tf_sample_predictions[users]).mean(dim=1)


class WARPLoss(LossGraph):
    """Extension (weighted approximate-rank pairwise loss, LightFM's 'warp'; not in the reference): the first-violator ranking loss
    over the static negative table WMRBLoss samples from.  For every stored interaction k of user u with a value > 0 and score p_k,
    the user's row sp[u, :] of sampled scores is tried in table order against the threshold t_k = p_k - 1 (rounded once in the dtype
    of the scores): sample s violates when sp[u, s] > t_k - strictly, and a NaN on either side never does.  With s* the first
    violator and N = s* + 1 the number of trials,

        w_k = log(max(1, floor((n_items - 1) / N)))        loss_k = w_k (1 - p_k + sp[u, s*])

    and loss_k = 0 where nothing violates or N > n_items - 1.  The weight is LightFM's rank estimate; it is a constant of the step
    (computed under no_grad), so d loss_k / d p_k = -w_k and d loss_k / d sp[u, s*] = w_k.  n_samples is the cap on trials
    (LightFM's max_sampled).  Stored values <= 0 take no part and a negative that coincides with one of the user's positives is
    not filtered (both as in WMRBLoss)."""

    def get_loss(self, tf_interactions, tf_sample_predictions, tf_prediction_serial, n_items, n_samples, predictions=None):
        mask = tf_interactions.values > 0.0
        users = tf_interactions.indices[:, 0][mask]
        pos = tf_prediction_serial[mask]
        sp = tf_sample_predictions[users]
        with torch.no_grad():
            violates = sp > (pos - 1.0)[:, None]
            found = violates.any(dim=1)
            first = violates.to(torch.uint8).argmax(dim=1)          # the first maximum: the first violator (0 where there is none)
            rank = torch.div(int(n_items) - 1, first + 1, rounding_mode='floor').clamp(min=1)
            w = torch.where(found, torch.log(rank.to(pos.dtype)), torch.zeros_like(pos))
        margin = 1.0 - pos + sp.gather(1, first[:, None])[:, 0]
        return torch.where(w > 0.0, w * margin, torch.zeros_like(pos))


class KOSWARPLoss(LossGraph):
    """Extension (the k-th order statistic loss of Weston, Yee and Weiss, modelled on LightFM's 'warp-kos'; not in the reference):
    WARPLoss pushes up every positive of a user, this loss the user's k-th best positive out of a draw of n.  LightFM draws the n
    positives at random; here the loss is the EXPECTATION over that draw, a weighted WARP without a random number.  For user u let
    E_u be its stored interactions with a value > 0 (duplicates as often as they are stored), P = |E_u|, n' = min(n, P) and
    k' = min(k, n').  For entry j of E_u with score p_j (compared in the dtype of the scores; a NaN orders below -inf and ties with
    the other NaNs):

        a_j = #{i in E_u : p_i > p_j}        b_j = #{i in E_u : p_i >= p_j}        B(q) = sum_{i < k'} C(n', i) q^i (1 - q)^(n' - i)
        omega_j = (B(a_j / P) - B(b_j / P)) / (b_j - a_j)        loss_j = omega_j w_j (1 - p_j + sp[u, s*_j])

    B(q) is the probability that fewer than k' of n' uniform draws with replacement land in a set of share q (B(0) = 1, B(1) = 0), so
    omega_j is the probability that the k'-th highest of the n' draws is j; a tie block shares its probability equally, and the
    weights of a user sum to 1: a user counts once, however many positives it has.  s*_j and w_j are exactly WARPLoss's first
    violator and weight.  omega_j and w_j are constants of the step (no_grad): d loss_j / d p_j = -omega_j w_j and
    d loss_j / d sp[u, s*_j] = omega_j w_j.  A user without positives contributes nothing.  k = n = 1 gives omega_j = 1 / P: the
    per-user mean of WARPLoss's terms.  1 <= k <= n <= 64 (ValueError)."""

    def __init__(self, k=5, n=10):
        for name, v in (('k', k), ('n', n)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f'KOSWARPLoss: {name}={v!r} is not an integer')
        if not 1 <= k <= n <= 64:
            raise ValueError(f'KOSWARPLoss: k={k}, n={n}: 1 <= k <= n <= 64')
        self.k, self.n = k, n

    def weights(self, users, pos, n_users):
        """omega per positive (users [E] int64, pos [E] scores) - a and b by sorting within users, B from its sum in pos.dtype."""
        with torch.no_grad():
            E, dt = pos.shape[0], pos.dtype
            if E == 0:
                return torch.zeros_like(pos)
            nan = torch.isnan(pos)
            x = torch.where(nan, torch.full_like(pos, -math.inf), pos)
            order = torch.sort(x, descending=True, stable=True)[1]               # by (user, a number before a NaN, score descending)
            order = order[torch.sort(nan[order].to(torch.uint8), stable=True)[1]]
            order = order[torch.sort(users[order], stable=True)[1]]
            xs, ns, us = x[order], nan[order], users[order]
            start = torch.ones(E, dtype=torch.bool, device=pos.device)           # the first entry of every tie block
            start[1:] = (us[1:] != us[:-1]) | (ns[1:] != ns[:-1]) | (xs[1:] != xs[:-1])
            block = torch.cumsum(start, 0) - 1
            block_first = torch.nonzero(start)[:, 0]
            block_size = torch.bincount(block)
            P_user = torch.bincount(users, minlength=n_users)
            user_first = torch.cumsum(P_user, 0) - P_user
            a = block_first[block] - user_first[us]
            b = a + block_size[block]
            P = P_user[us]
            np_, i = P.clamp(max=self.n), torch.arange(self.k, device=pos.device)
            kp = np_.clamp(max=self.k)
            comb = torch.tensor([[math.comb(m, j) for j in range(self.k)] for m in range(self.n + 1)], dtype=dt, device=pos.device)

            def B(c):
                q, r = (c.to(dt) / P.to(dt))[:, None], ((P - c).to(dt) / P.to(dt))[:, None]
                terms = comb[np_] * q ** i * r ** (np_[:, None] - i).clamp(min=0)
                return torch.where(i[None, :] < kp[:, None], terms, torch.zeros_like(terms)).sum(dim=1)
            omega = ((B(a) - B(b)) / (b - a).to(dt)).clamp(min=0.0)
            out = torch.empty_like(pos)
            out[order] = omega
            return out

    def get_loss(self, tf_interactions, tf_sample_predictions, tf_prediction_serial, n_items, n_samples, predictions=None):
        mask = tf_interactions.values > 0.0
        users = tf_interactions.indices[:, 0][mask]
        omega = self.weights(users, tf_prediction_serial[mask].detach(), tf_sample_predictions.shape[0])
        return omega * WARPLoss().get_loss(tf_interactions=tf_interactions, tf_sample_predictions=tf_sample_predictions,
                                           tf_prediction_serial=tf_prediction_serial, n_items=n_items, n_samples=n_samples)


class SampledSoftmaxLoss(LossGraph):
    """Extension (the sampled softmax of retrieval models; not in the reference): the softmax of a positive against the user's row of
    the static negative table WMRBLoss samples from.  For every stored interaction k of user u with a value > 0 and score p_k, against
    the user's row sp[u, :] of sampled scores:

        loss_k = -log( exp(p_k) / (exp(p_k) + c sum_s exp(sp[u, s])) )        c = 1, or n_items / n_samples with ``catalog_scale``

    With ``catalog_scale`` c is the constant WMRBLoss uses: the uniform-sampling correction that makes the sum an estimate of the
    full-catalog partition.  d loss_k / d p_k = -(1 - q_k) and d loss_k / d sp[u, s] = c exp(sp[u, s]) / (exp(p_k) + c sum_s' exp(sp[u, s']))
    with q_k the probability inside the logarithm: every sample pulls, the higher it scores the harder.  Stored values <= 0 take
    no part and a negative that coincides with one of the user's positives is not filtered (both as in WMRBLoss)."""

    def __init__(self, catalog_scale=False):
        self.catalog_scale = bool(catalog_scale)

    def get_loss(self, tf_interactions, tf_sample_predictions, tf_prediction_serial, n_items, n_samples, predictions=None):
        mask = tf_interactions.values > 0.0
        users = tf_interactions.indices[:, 0][mask]
        pos = tf_prediction_serial[mask]
        log_c = math.log(n_items / n_samples) if self.catalog_scale else 0.0
        partition = torch.logsumexp(tf_sample_predictions, dim=1)[users] + log_c     # log(c sum_s exp(sp[u, s])), per positive
        return torch.logaddexp(pos, partition) - pos


class FullSoftmaxLoss(LossGraph):
    """Extension (the softmax the sampled losses approximate; not in the reference): the softmax of a positive against EVERY item of
    the catalog.  For every stored interaction k of user u with a value > 0 and score p_k:

        loss_k = logsumexp_i(predictions[u, :]) - p_k

    The positive itself is part of the partition, and so is every other positive of the user.  Stored values <= 0 take no part (as
    in WMRBLoss); a duplicate counts as often as it is stored.  With pi_ui = exp(s_ui - lse_u) and n_u the number of stored entries
    of u with a value > 0, the gradient of the sum over positives is  n_u pi_ui - [number of positives of u at i]  per score: dense
    on the item side (every item row moves when any user has a positive), zero for a user without positives.  No negative table, no
    n_samples, no resampling: the engine sweeps U V^T through the matrix cores without materialising it; this is the definition."""

    def get_loss(self, tf_interactions, predictions, tf_sample_predictions=None, tf_prediction_serial=None, n_items=None,
                 n_samples=None):
        mask = tf_interactions.values > 0.0
        users = tf_interactions.indices[:, 0][mask]
        items = tf_interactions.indices[:, 1][mask]
        return torch.logsumexp(predictions, dim=1)[users] - predictions[users, items]
