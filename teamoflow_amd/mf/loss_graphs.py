"""Loss graphs (plug-in interface of /root/reference/src/teamoflow/mf/loss_graphs.py).

``MSELoss``, ``WMRBLoss``, ``KLDivergenceLoss``, ``LogisticLoss``, ``BPRLoss``, ``WARPLoss``, ``SampledSoftmaxLoss`` and
``FullSoftmaxLoss`` (extensions: the reference has no logistic loss, pointwise or pairwise, no first-violator ranking loss and no
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
