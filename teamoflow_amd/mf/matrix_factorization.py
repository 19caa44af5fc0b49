"""``MatrixFactorization`` with the class surface of
/root/reference/src/teamoflow/mf/matrix_factorization.py:23-475, computed sparsely on MI355X.

Dispatch (``MatrixFactorization._route``; same isinstance test the reference uses at :115,:136-162): a model made of
(``LinearEmbedding`` | ``BiasedLinearEmbedding``) x indicator features x a loss of the table ``_engine.LOSSES`` (``ENGINE_LOSSES``) - or
``LinearEmbedding`` over ``SparseFeatures`` on either side, or with ``relu_engine = True``
(off by default) a ``ReLUEmbedding`` side over either - trains on the HIP engine (``_engine.py`` -> libtmf.so); for unbiased MSE / WMRB it
needs a GPU - there is no CPU fallback for them.  Any other combination of plug-ins (dense features, ReLU embeddings, user subclasses)
trains through ``_fit_generic``: the reference's dense loop written with torch autograd around the plug-ins' own ``get_repr`` /
``get_loss`` - and so does KL on a table with an empty class.  Which settings (no GPU, ``batch_users``, ``shard_items``, ``data_parallel``,
bf16 storage, ``optimizer='adam'``) keep an engine model on the engine, hand it to the generic loop (a side over ``SparseFeatures`` then
as a dense matrix) or are refused with ``NotImplementedError`` is the table ``ROUTES`` below.
``user_alpha`` / ``item_alpha`` > 0 (extensions, off by default) add ``alpha ||W_side||_F^2`` to the objective on either path: on the engine
through the ``_l2`` twins of the table steps (``_engine.TrainState.set_l2``), in the generic loop as a term of the differentiated sum.
``fit_als`` (an extension) trains the same tables by alternating least squares instead of gradient steps, and ``fold_in_users`` /
``fold_in_items`` embed rows that arrived after a fit from their interactions (``teamoflow_amd/_als.py``, ``csrc/tmf_als.hip``).
"""
import copy
import os
import timeit
import warnings

import numpy as np
import torch

from .. import _als, _engine, _lib, _ops
from .embedding_graphs import BiasedLinearEmbedding, Embeddings, LinearEmbedding, ReLUEmbedding
from .initializer_graphs import NormalInitializer
from .loss_graphs import LossGraph, MSELoss  # noqa: F401  (what the engine knows of every other loss is _engine.LOSSES)
from .sparse import IndicatorFeatures, SparseFeatures, SparseInteractions, default_device, is_indicator
from .utils import gather_matrix_indices, log_expected_count, popularity_weights, random_sampler, random_sampler_device

PREDICT_CHUNK_BYTES = 2 << 30  # users are scored in blocks of at most this many bytes of scores
HOST_SAMPLER_MAX_WORK = 2_000_000_000  # n_users * n_items above which generate_sample=True samples on the device
GRAPH_EPOCHS = 50              # epochs captured per hipGraph on launch-bound problems
GRAPH_MAX_WORK = 20_000_000    # interactions + sampled scores per epoch below which fit() uses graphs


def _loss_classes(keep=lambda rec: True):
    return tuple(dict.fromkeys(rec.cls for rec in _engine.LOSSES.values() if keep(rec)))   # in the table's order, each class once


# What trains where (DESIGN.md prints this table; MatrixFactorization._route reads it).  A row is a feature of a fit, a column a
# setting that leaves the single-GPU full-batch fp32 fresh-Adam fit: 'ok' = the engine has that form, 'generic' = fit() trains
# through _fit_generic, 'refuse' = NotImplementedError before any weight is drawn or plan built.
ENGINE_LOSSES = _loss_classes()                                     # exactly these types, no subclass
TABLE_LOSSES = _loss_classes(lambda rec: rec.table)                 # these and their subclasses read the static negative table
PAIR_STEP_LOSSES = _loss_classes(lambda rec: rec.sliced_only)       # the route feature 'pair': a pair step of the sliced user pass
PAIR_ROW_LOSSES = _loss_classes(lambda rec: rec.route == 'pair')    # the losses that answer by the row 'pair': single GPU, full batch
_FEEDS = {feeds: _loss_classes(lambda rec: rec.feeds == feeds) for feeds in ('samples', 'serial')}   # Loss.feeds -> these and their subclasses
_SETTINGS = {   # column -> (the attribute a refusal names, has the model left its default?), in the order refusals are met
    'relu_engine': ('relu_engine', lambda m: getattr(m, 'relu_engine', 0)     # counts beside a ReLUEmbedding side only
                    and ReLUEmbedding in (type(m.user_repr_graph), type(m.item_repr_graph))),
    'batch_users': ('batch_users', lambda m: getattr(m, 'batch_users', 0)),
    'shard_items': ('shard_items', lambda m: getattr(m, 'shard_items', 0)),
    'data_parallel set': ('data_parallel', lambda m: getattr(m, 'data_parallel', 0)),      # the attribute, with or without ranks
    'data_parallel active': ('data_parallel', lambda m: m._data_parallel_active()),        # more than one rank, or 'force'
    'bf16': ('factor_dtype', lambda m: m.factor_dtype is not torch.float32),
    'adam': ('optimizer', lambda m: m.optimizer != 'fresh_adam'),
    'no GPU': (None, lambda m: not torch.cuda.is_available()),
}
ROUTES = {feature: dict(zip(_SETTINGS, row.split(), strict=True)) for feature, row in {
    # feature     relu_engine  batch_users  shard_items  dp set   dp active  bf16     adam     no GPU
    'kl':        'ok           generic      generic      ok       generic    ok       ok       generic',   # KLDivergenceLoss
    'pair':      'ok           refuse       refuse       refuse   refuse     ok       ok       generic',   # PAIR_STEP_LOSSES
    'logistic':  'ok           ok           ok           ok       ok         ok       ok       generic',   # LogisticLoss
    'side':      'ok           generic      generic      ok       generic    generic  generic  generic',   # biased, SparseFeatures, ReLU
    'l2':        'refuse       refuse       refuse       refuse   refuse     ok       ok       ok',        # user_alpha / item_alpha > 0
    'resample':  'ok           refuse       refuse       refuse   refuse     ok       ok       ok',        # resample_every on a table loss
    'als':       'ok           refuse       refuse       refuse   refuse     refuse   ok       ok',        # fit_als
}.items()}
_BUILT = {'pair': 'only the single-GPU full-batch fit is built for this loss',
          'l2': 'L2 regularisation is built for the single-GPU full-batch fit and the generic loop only',
          'resample': 'the negative table is resampled in the single-GPU full-batch fit and the generic loop only',
          'als': 'only the single-GPU full-batch fit is built, and its regulariser is reg',
          'item_bias': 'the scalar item bias is built for the single-GPU full-batch fit on float32 tables and the generic loop only',
          'popularity': 'the negative table is drawn by popularity in the single-GPU full-batch fit and the generic loop only',
          'logq': 'the logQ correction is built for the single-GPU full-batch fit and the generic loop only'}
#                                                                                      how a refusal ends, per feature
# scalar_item_bias = True, a table of its own beside ROUTES (DESIGN.md prints both; _route reads both): the settings the bias is
# refused with whatever the trainer, and the families of _engine.LOSSES whose engine epoch has the two bias passes.  A loss that is
# no engine loss (a subclass, a plug-in) trains its bias in the generic loop
ITEM_BIAS_ROUTES = {'item_bias': dict(zip(_SETTINGS, 'ok refuse refuse refuse refuse refuse ok ok'.split(), strict=True))}
ITEM_BIAS_FAMILIES = {'table': 'ok', 'list': 'refuse', 'catalog': 'refuse'}
# negative_sampling = 'popularity' on a table loss, a table of its own like the bias's: the forms that draw their tables themselves
# are where 'resample' is refused, and so is this.  With 'uniform' or without the attribute it is never looked at
SAMPLING_ROUTES = {'popularity': dict(ROUTES['resample'])}
NEGATIVE_SAMPLING = ('uniform', 'popularity')
# sampling_correction = 'logq' on SampledSoftmaxLoss (and its subclasses), a table of its own like the two above and refused exactly
# where 'popularity' is: the forms that draw their tables themselves know neither the weights nor the offsets.  With 'none' or without
# the attribute, or on a loss that reads no negative table, it is never looked at
CORRECTION_ROUTES = {'logq': dict(SAMPLING_ROUTES['popularity'])}
SAMPLING_CORRECTION = ('none', 'logq')


def augmented_tables(user_embedding, item_embedding, item_bias):
    """([U | 1], [V | b], fused): the tables whose product is U V^T + 1 b^T - the ONE place the ranking calls of a model with a scalar
    item bias get their operands from (MatrixFactorization._score_tables).  float32 [rows, r + 1] views of fresh tables whose rows are
    padded to 16 bytes; the column of ones and b are exact in every arithmetic of the fused kernels (1.0 is its own first bf16 plane,
    b splits into its three planes like any factor).  fused: whether the width r + 1 still fits the fused ranking kernels (r + 1 <=
    _ops.FUSED_MAX_R); a wider model ranks through predict_gemm + topk_stable and the block form of item_ranks."""
    (m, r), n = user_embedding.shape, item_embedding.shape[0]
    ld, dev = (r + 1 + 3) // 4 * 4, user_embedding.device
    Ua = torch.zeros(m, ld, dtype=torch.float32, device=dev)
    Va = torch.zeros(n, ld, dtype=torch.float32, device=dev)
    Ua[:, :r], Va[:, :r] = user_embedding.detach(), item_embedding.detach()
    Ua[:, r] = 1.0
    Va[:, r] = item_bias.detach().to(dev)
    return Ua[:, :r + 1], Va[:, :r + 1], r + 1 <= _ops.FUSED_MAX_R


class SampleTableMissing(AttributeError):
    """The losses of the table family (TABLE_LOSSES) need the static negative table: build the model with generate_sample=True
    (the reference fails with AttributeError inside gather_matrix_indices, matrix_factorization.py:153)."""


def _as_interactions(x):
    if isinstance(x, SparseInteractions):
        return x
    if hasattr(x, 'indices') and hasattr(x, 'values') and hasattr(x, 'dense_shape'):
        return SparseInteractions(x.indices, x.values, tuple(int(d) for d in x.dense_shape))
    from .input_utils import convert_to_sparse
    return convert_to_sparse(x)


class MatrixFactorization:
    """Standard matrix factorization with pluggable embedding / loss / initializer graphs."""

    def __init__(self, n_components, user_repr_graph=LinearEmbedding(), item_repr_graph=LinearEmbedding(),
                 loss_graph=MSELoss(), user_weight_graph=NormalInitializer(), item_weight_graph=NormalInitializer(),
                 n_users=None, n_items=None, n_samples=None, generate_sample=False):
        self.n_components = n_components
        self.user_repr_graph = user_repr_graph
        self.item_repr_graph = item_repr_graph
        self.loss_graph = loss_graph
        self.user_weight_graph = user_weight_graph
        self.item_weight_graph = item_weight_graph

        self.n_users = n_users
        self.n_items = n_items
        self.n_samples = n_samples
        self.random_ind = None
        self.generate_sample = generate_sample
        if n_samples is None and n_items is not None:  # :68-69
            self.n_samples = n_items // 2
        if generate_sample == True:  # noqa: E712  (:72-73; the table is drawn once and never resampled)
            if n_users * n_items > HOST_SAMPLER_MAX_WORK and torch.cuda.is_available():
                # the reference's host loop (one O(n_items) np.random.choice per user) would take minutes here:
                # draw the table on the device instead - same distribution, not the NumPy stream
                warnings.warn(f'random_sampler: {n_users} users x {n_items} items is too large for the host loop; '
                              'drawing the negative table on the device (utils.random_sampler_device)')
                self.random_ind = random_sampler_device(n_items, n_users, self.n_samples)
            else:
                self.random_ind = random_sampler(n_items, n_users, self.n_samples)

        if isinstance(self.user_repr_graph, ReLUEmbedding):  # :76-79
            self.user_aux_dim = 5 * self.n_components
        if isinstance(self.item_repr_graph, ReLUEmbedding):
            self.item_aux_dim = 5 * self.n_components
        self.user_relu_bias = None
        self.user_relu_weight = None
        self.item_relu_bias = None
        self.item_relu_weight = None
        self.user_linear_bias = None
        self.item_linear_bias = None
        self.user_trainable = None
        self.item_trainable = None

        self.loss_history_ = []   # extension: mean loss of every epoch of the last fit
        self.fit_seconds_ = 0.0   # extension: time spent in the epoch loop of the last fit
        self.plan_seconds_ = 0.0  # extension: time spent building the index structures of the last fit
        self.graph_epochs_ = 0    # extension: epochs of the last fit that ran as replays of a captured hipGraph (0: every one launched)
        self.verbose = True
        self.factor_dtype = torch.float32  # extension: torch.bfloat16 = bf16 factor storage, fp32 arithmetic
        self.predict_arithmetic = None     # extension: 'auto' (default: 'split' or 'fp32', both on whole fp32 factors) | 'fp32' | 'split' | 'half2' (opt-in, 22 bits) - _ops.predict_topk
        self.data_parallel = False         # extension: split the users over torch.distributed ranks (teamoflow_amd/dist.py)
        # extension: q >= 1 = item-row-sharded V in q windows per rank (dist.fit_item_sharded): the item table is owned in
        # row blocks and streamed window by window instead of being replicated - for catalogs beyond one GPU's memory
        self.shard_items = 0
        # extension, OFF by default (the reference is full-batch): B > 0 = one optimiser step per batch of B users
        # (teamoflow_amd/_minibatch.py)
        self.batch_users = 0
        # extension, OFF by default: 'adam' keeps Adam's moments across epochs.  The reference (and the default here,
        # 'fresh_adam') builds a new optimizer every epoch (:176), i.e. every step is Adam's first step.
        self.optimizer = 'fresh_adam'
        # extension, OFF by default: True = a ReLUEmbedding side over eye() or SparseFeatures trains on the HIP engine
        # (_engine.ReLUSide / epoch_sides) where a biased side would; False = the generic path, as before
        self.relu_engine = False
        # extension, OFF by default (the reference has no regularisation): the objective whose gradient a fit takes gains
        # user_alpha ||W_user||_F^2 + item_alpha ||W_item||_F^2 over the sides' weight matrices (never a bias); loss_history_ stays
        # the data term.  The penalty stands against the gradient of a SUM over interactions: a useful alpha grows with the
        # interactions per row
        self.user_alpha = 0.0
        self.item_alpha = 0.0
        # extension, OFF by default (the reference trains on ONE negative table): k > 0 = a fit of one of the TABLE_LOSSES trains
        # epoch e on the table of round j = e // k - round 0 on random_ind as it stands, round j >= 1 on
        # _ops.sample_negatives(n_items, n_users, n_samples of random_ind, seed=sample_seed + j) (LightFM and implicit draw fresh
        # negatives every step).  random_ind itself is never changed, so every fit starts again from round 0.  Losses that read no
        # table (MSE, KL, Logistic) are not affected.  Full-batch on one GPU, or the generic loop
        self.resample_every = 0
        self.sample_seed = 0
        self.resample_rounds_ = 0     # tables the last fit trained on, round 0's included (0: its loss reads no table)
        self.resample_seconds_ = 0.0  # time the last fit spent drawing tables and rebuilding their plans (part of fit_seconds_)
        # extension, OFF by default (the reference's table is uniform over the catalog): 'popularity' = a fit of one of the
        # TABLE_LOSSES draws EVERY round's table, round 0's included, with item i weighted (c_i + 1)^sampling_power, c_i the number
        # of training entries of item i with a value > 0 (word2vec's unigram^0.75; implicit's BPR): round j trains on
        # _ops.sample_negatives(n_items, n_users, S, seed=sample_seed + j, weights=utils.popularity_weights(c, sampling_power)).
        # random_ind is still required, gives S, and is never changed.  The losses read the table as they read a uniform one.
        # Full-batch on one GPU, or the generic loop (SAMPLING_ROUTES); losses that read no table are not affected
        self.negative_sampling = 'uniform'
        self.sampling_power = 0.75
        # extension, OFF by default: 'logq' = a SampledSoftmaxLoss fit subtracts from every sampled logit the log of how often the
        # sampler proposes that item, l_i = utils.log_expected_count(q, S)[i] - loss_k = logaddexp(p_k, logsumexp_s(sp[u, s] -
        # l[R[u, s]])) - p_k, the positive keeps its raw score - so that the sum over the samples estimates the full-catalog
        # partition again whatever the proposal (the sampled-softmax / logQ correction of retrieval models).  Under 'uniform' l is the
        # constant log(S / n_items) and the fit IS SampledSoftmaxLoss(catalog_scale=True), bit for bit; under 'popularity' l comes
        # from the fit's weights, once per fit, and stays in sample_log_q_.  Only the training loss sees it: predict and the ranking
        # calls do not.  The other table losses refuse it (CORRECTION_ROUTES; losses that read no table are not affected)
        self.sampling_correction = 'none'
        self.sample_log_q_ = None     # l of the last fit: float32 [n_items] on the CPU (None: the fit built no table of offsets)
        # extension, OFF by default (the reference's score is U[u] . V[i]): True = one trainable scalar per item beside its factor
        # (LightFM's item_biases), score U[u] . V[i] + item_bias_[i] in the loss and in every ranking call.  Starts from zeros at
        # every fit, takes the optimiser's step like any other variable and is never penalised.  On the engine for the table family
        # (_engine.ItemScalarBias), else in the generic loop; what it is refused with: ITEM_BIAS_ROUTES / ITEM_BIAS_FAMILIES
        self.scalar_item_bias = False
        self.item_bias_ = None        # the trained bias of the last fit: float32 [n_items] on the tables' device (None: it had none)

    # ------------------------------------------------------------------------------------------
    # training
    # ------------------------------------------------------------------------------------------
    def _data_parallel_active(self):
        return bool(self.data_parallel and torch.distributed.is_available() and torch.distributed.is_initialized()
                    and torch.distributed.get_world_size() > 1 or (self.data_parallel == 'force'))

    def _answer(self, feature, what=None, also=(), table=ROUTES):
        """'engine', or 'generic' / NotImplementedError for the first setting, in ROUTES' column order, that this model has left the
        default of and ``feature`` has no engine form for.  what: a refusal's name for the feature; also: attributes refused when set;
        table: the table ``feature`` is a row of."""
        def refuse(name):
            raise NotImplementedError(f'{what} with {name}={getattr(self, name)!r}: {_BUILT[feature]} (set {name} back to its default)')
        for setting, (name, left) in _SETTINGS.items():
            answer = table[feature][setting]
            if answer != 'ok' and left(self):
                return 'generic' if answer == 'generic' else refuse(name)
        for name in also:
            if getattr(self, name, 0):
                refuse(name)
        return 'engine'

    def _route(self, user_features, item_features):
        """'engine' | 'generic': the trainer of this fit, after the refusals (NotImplementedError; ValueError for a bad user_alpha /
        item_alpha / resample_every / sample_seed / negative_sampling / sampling_power / sampling_correction) - the one place that decides either, from
        ROUTES.  Nothing is drawn or built here.
        The engine takes exactly the ENGINE_LOSSES over sides that are exactly LinearEmbedding / BiasedLinearEmbedding over indicator
        features or LinearEmbedding over SparseFeatures with entries (with relu_engine also exactly ReLUEmbedding over either, while
        its aux width 5 r fits a table row) when no feature of the fit answers 'generic'.  Unbiased MSE / WMRB have no row in ROUTES:
        every setting is a form of theirs, and without a GPU they fail in _fit_sparse - there is no CPU fallback."""
        loss, kinds = type(self.loss_graph), (type(self.user_repr_graph), type(self.item_repr_graph))
        rec = next((rec for rec in _engine.LOSSES.values() if rec.cls is loss), None)   # a class's records share route and family
        row = rec.route if rec else None
        if self._item_bias_setting():   # the setting's own refusals (ITEM_BIAS_ROUTES, ITEM_BIAS_FAMILIES), whatever the trainer
            self._answer('item_bias', 'scalar_item_bias=True', table=ITEM_BIAS_ROUTES)
            if rec is not None and ITEM_BIAS_FAMILIES[rec.family] != 'ok':
                raise NotImplementedError(f'scalar_item_bias=True with {loss.__name__}: the engine adds the bias to the scores of the '
                                          f'table family only ({", ".join(c.__name__ for c in TABLE_LOSSES)}); the passes of the other '
                                          f'engine losses form their scores inside the kernels (set scalar_item_bias back to its default)')
        if self._sampling_setting()[0] == 'popularity':   # the setting's own refusals (SAMPLING_ROUTES); None for a loss without a table
            self._answer('popularity', "negative_sampling='popularity'", table=SAMPLING_ROUTES)
        if self._correction_setting() == 'logq':   # the setting's own refusals (CORRECTION_ROUTES); 'none' for a loss without a table
            softmax = _engine.LOSSES['softmax'].cls
            if not isinstance(self.loss_graph, softmax):
                raise NotImplementedError(f"sampling_correction='logq' with {loss.__name__}: the correction is built for "
                                          f'{softmax.__name__} only - an importance-weighted hinge and a rank estimate under a '
                                          f'proposal are different mathematics (set sampling_correction back to its default)')
            if getattr(self.loss_graph, 'catalog_scale', False):
                raise ValueError(f"sampling_correction='logq' with {loss.__name__}(catalog_scale=True): the correction contains that "
                                 f'constant (under uniform sampling it is exactly it) - use one of the two')
            self._answer('logq', "sampling_correction='logq'", table=CORRECTION_ROUTES)
        # the refusals, in the order a model that meets several has always met them
        answers = [self._answer('pair', loss.__name__)] if row == 'pair' else []
        if any(self._alphas()):
            self._answer('l2', 'user_alpha / item_alpha > 0')
        every = self._resample_setting()[0]
        if every:
            self._answer('resample', f'resample_every={every}')
        relu = getattr(self, 'relu_engine', False) and 5 * self.n_components <= 1024
        linear = (LinearEmbedding, ReLUEmbedding) if relu else (LinearEmbedding,)
        featured = [isinstance(f, SparseFeatures) for f in (user_features, item_features)]
        if not (loss in ENGINE_LOSSES
                and all((kind in linear and f.nnz > 0) if sparse else (kind in linear + (BiasedLinearEmbedding,) and is_indicator(f))
                        for kind, f, sparse in zip(kinds, (user_features, item_features), featured))):
            return 'generic'
        structured = any(featured) or BiasedLinearEmbedding in kinds or ReLUEmbedding in kinds
        answers += [self._answer(feature) for feature, there in ((row, row not in (None, 'pair')), ('side', structured)) if there]
        if 'generic' in answers:
            return 'generic'
        if rec.family == 'catalog':
            # the sweep kernels' own limits.  Refused, not handed to the generic loop: its [m, n] matrix is what this loss avoids
            if self.factor_dtype is not torch.float32:
                raise NotImplementedError(f'FullSoftmaxLoss with factor_dtype={self.factor_dtype}: its kernels sweep float32 tables '
                                          f'only (set factor_dtype back to torch.float32)')
            if self.n_components > _engine.FULL_SOFTMAX_MAX_COMPONENTS:
                raise NotImplementedError(f'FullSoftmaxLoss with n_components={self.n_components} > {_engine.FULL_SOFTMAX_MAX_COMPONENTS}: '
                                          f'the sweep kernel holds a 128-row tile of the swept table in LDS beside its output '
                                          f'accumulators; wider models are not built')
        return 'engine'

    def _engine_form(self):
        """Which fit _fit_sparse runs: 'batch_users' | 'shard_items' | 'data_parallel' | 'full'.  The forms exclude each other:
        batch_users beside either of the others is a ValueError, raised as before when the engine fit starts."""
        if getattr(self, 'batch_users', 0):
            if getattr(self, 'shard_items', 0) or self.data_parallel:
                raise ValueError('batch_users cannot be combined with shard_items / data_parallel')
            return 'batch_users'
        if getattr(self, 'shard_items', 0):
            return 'shard_items'
        return 'data_parallel' if self._data_parallel_active() else 'full'

    def _alphas(self):
        """(user_alpha, item_alpha) as floats, checked: negative or non-finite raises ValueError."""
        out = []
        for name in ('user_alpha', 'item_alpha'):
            try:
                a = float(getattr(self, name, 0.0))
            except (TypeError, ValueError):
                raise ValueError(f'{name}={getattr(self, name)!r} is not a number') from None
            if not 0.0 <= 2.0 * a <= float(np.finfo(np.float32).max):   # 2 alpha travels as an fp32 scalar; NaN fails both comparisons
                raise ValueError(f'{name}={a!r}: the L2 penalty must be finite and >= 0')
            out.append(a)
        return tuple(out)

    def _item_bias_setting(self):
        """scalar_item_bias as a bool (False on a model that never had the attribute); anything but a bool raises ValueError."""
        v = getattr(self, 'scalar_item_bias', False)
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f'scalar_item_bias={v!r}: True or False')
        return bool(v)

    def _resample_setting(self):
        """(resample_every, sample_seed) as ints, checked (ValueError: negative or not an integer) - resample_every as 0 for a loss that
        reads no negative table.  The forms that cannot resample are refused by _route (ROUTES['resample'])."""
        out = []
        for name in ('resample_every', 'sample_seed'):
            v = getattr(self, name, 0)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or (name == 'resample_every' and v < 0):
                raise ValueError(f'{name}={v!r}: an integer' + (' >= 0 (0 = never resample)' if name == 'resample_every' else ''))
            out.append(int(v))
        if not isinstance(self.loss_graph, TABLE_LOSSES):
            return 0, out[1]
        return tuple(out)

    def _sampling_setting(self):
        """(negative_sampling, sampling_power), checked (ValueError: a name that is not one of NEGATIVE_SAMPLING; under 'popularity' a
        power that is not finite and >= 0) - ('uniform' on a model that never had the attribute) and (None, power) for a loss that
        reads no negative table.  The forms that cannot draw by popularity are refused by _route (SAMPLING_ROUTES)."""
        how, power = getattr(self, 'negative_sampling', 'uniform'), getattr(self, 'sampling_power', 0.75)
        if not isinstance(how, str) or how not in NEGATIVE_SAMPLING:
            raise ValueError(f"negative_sampling={how!r}: 'uniform' or 'popularity'")
        if how == 'popularity':
            if isinstance(power, bool) or not isinstance(power, (int, float, np.integer, np.floating)) \
                    or not (np.isfinite(power) and power >= 0):
                raise ValueError(f'sampling_power={power!r}: a finite number >= 0')
            power = float(power)
        return (how if isinstance(self.loss_graph, TABLE_LOSSES) else None), power

    def _correction_setting(self):
        """sampling_correction, checked (ValueError: not one of SAMPLING_CORRECTION) - 'none' on a model that never had the attribute
        and for a loss that reads no negative table.  What 'logq' is refused with: _route (CORRECTION_ROUTES)."""
        how = getattr(self, 'sampling_correction', 'none')
        if not isinstance(how, str) or how not in SAMPLING_CORRECTION:
            raise ValueError(f"sampling_correction={how!r}: 'none' or 'logq'")
        return how if isinstance(self.loss_graph, TABLE_LOSSES) else 'none'

    def _sample_log_q(self):
        """l of a fit under sampling_correction='logq' whose tables are drawn by popularity (float32 [n_items] on the CPU:
        utils.log_expected_count of the fit's weights and the S of random_ind), else None - under 'uniform' the correction is the
        constant c = n_items / n_samples and no table exists.  Once per fit, after _popularity_weights."""
        q = getattr(self, '_sampling_weights', None)
        if self._correction_setting() != 'logq' or q is None or self.random_ind is None:
            return None
        return log_expected_count(q, int(torch.as_tensor(self.random_ind).shape[1]))

    def _popularity_weights(self, interactions, n_items):
        """The weights of this fit's tables under negative_sampling='popularity' (int64 [n_items], on the CPU), else None: c_i = the
        stored entries of item i with a value > 0, q = utils.popularity_weights(c, sampling_power).  Once per fit."""
        how, power = self._sampling_setting()
        if how != 'popularity':
            return None
        items = interactions.indices[:, 1][interactions.values > 0].to(torch.int64)
        return popularity_weights(torch.bincount(items, minlength=n_items).cpu(), power)

    def _draw_round(self, j, n_items, n_users, dev):
        """The table of round j (int32, on dev): a function of (sample_seed + j, shape) alone - under negative_sampling='popularity'
        of the fit's weights too, and then for every j >= 0; else for j >= 1."""
        S = int(torch.as_tensor(self.random_ind).shape[1])
        q = getattr(self, '_sampling_weights', None)
        if q is not None:
            return _ops.sample_negatives(n_items, n_users, S, seed=self._resample_setting()[1] + j, device=dev, weights=q)
        return _ops.sample_negatives(n_items, n_users, S, seed=self._resample_setting()[1] + j, device=dev)

    def _reset_fit_products(self, sparse_feature_sides):
        """What one fit keeps for the calls after it and the next fit must not inherit (fit and fit_als share it): the sharded epoch
        of the last fit and the per-side records embed_users / embed_items read.  The variables the reference carries from fit to
        fit (user_linear_bias, user_relu_weight, ... - a later biased or ReLU fit starts from them) stay, and so does ``_state``,
        whose presence says that some fit of this model ran on the engine (fit_als, which has no engine state, drops it)."""
        self._sharded_epoch = None
        self._sparse_feature_sides = tuple(sparse_feature_sides)
        self._feature_weights = [None, None]   # padded engine weights of a side trained over SparseFeatures (embed_users / embed_items)
        self._relu_sides = [None, None]        # the _engine.ReLUSide of a ReLU side trained on the engine (embed_users / embed_items)
        self._sampling_weights = None          # the weights of a fit under negative_sampling='popularity' (fit sets them)
        self.sample_log_q_ = None              # the offsets of a fit under sampling_correction='logq' on such tables (likewise)

    def fit(self, epochs, user_features, item_features, tf_interactions, lr=1e-2):
        """matrix_factorization.py:96-187.  Re-initialises the weights on every call, runs ``epochs``
        full-batch steps (loss -> gradient of the SUM of the per-interaction losses -> a fresh Adam
        step), then stores user_embedding / item_embedding / *_trainable.  Returns None."""
        route = self._route(user_features, item_features)   # and the refusals: before any weight is drawn or plan built
        self.resample_rounds_, self.resample_seconds_, self.graph_epochs_ = 0, 0.0, 0
        self.item_bias_ = None   # a fit with scalar_item_bias leaves its bias here; every fit starts it from zeros
        n_users, n_user_features = user_features.shape
        n_items, n_item_features = item_features.shape
        if not isinstance(self.user_repr_graph, ReLUEmbedding):
            U = self.user_weight_graph.initialize_weights(n_user_features, self.n_components)
        else:
            U = self.user_weight_graph.initialize_weights(self.user_aux_dim, self.n_components)
        if not isinstance(self.item_repr_graph, ReLUEmbedding):
            V = self.item_weight_graph.initialize_weights(n_item_features, self.n_components)
        else:
            V = self.item_weight_graph.initialize_weights(self.item_aux_dim, self.n_components)
        interactions = _as_interactions(tf_interactions)
        self._reset_fit_products((isinstance(user_features, SparseFeatures), isinstance(item_features, SparseFeatures)))
        self._sampling_weights = self._popularity_weights(interactions, n_items)
        self.sample_log_q_ = self._sample_log_q()
        if route == 'engine':
            feats = [f if sparse else None for f, sparse in zip((user_features, item_features), self._sparse_feature_sides)]
            if self._fit_sparse(epochs, n_users, n_items, interactions, lr, U, V, *feats):
                return
        # the generic loop multiplies dense matrices: SparseFeatures works there as its dense form does
        user_features, item_features = (f.to_dense(W.device) if isinstance(f, SparseFeatures) else f
                                        for f, W in ((user_features, U), (item_features, V)))
        self._fit_generic(epochs, user_features, item_features, interactions, lr, U, V)

    # ------------------------------------------------------------------------------------------
    # alternating least squares (extension: teamoflow_amd/_als.py)
    # ------------------------------------------------------------------------------------------
    def _check_als_kernel(self, what, solver='cholesky'):
        """ALS solves fp32 tables of at most 128 components (solver='cg': 256): the row-solve kernels' limits (forms: ROUTES['als'])."""
        if solver == 'cg' and self.n_components > _als.CG_MAX_COMPONENTS:
            raise NotImplementedError(f"{what}: n_components={self.n_components} > {_als.CG_MAX_COMPONENTS} - the conjugate-gradient "
                                      f'kernel holds a row in the registers of eight lanes; wider models are not built')
        if solver != 'cg' and self.n_components > _als.MAX_COMPONENTS:
            raise NotImplementedError(f'{what}: n_components={self.n_components} > {_als.MAX_COMPONENTS} - the per-row factorisation '
                                      f"holds an r x r matrix in LDS; solver='cg' takes up to {_als.CG_MAX_COMPONENTS} components")
        if self.factor_dtype is torch.bfloat16 and what == 'fit_als':
            raise NotImplementedError('fit_als: factor_dtype=torch.bfloat16 - the normal equations are solved on float32 tables only')

    def fit_als(self, epochs, user_features, item_features, tf_interactions, *, reg=0.01, alpha=1.0, implicit=True,
                solver='cholesky', cg_steps=3):
        """Extension (implicit's AlternatingLeastSquares; Hu, Koren and Volinsky): ``epochs`` sweeps of alternating least squares
        instead of gradient steps - no learning rate, and converged after 10 - 20 sweeps.  Leading arguments as ``fit``.
        implicit=True: confidence 1 + alpha |a| on every stored value a, preference 1 where a > 0 and 0 everywhere else (all
        unstored pairs included; a stored 0 changes nothing, a stored negative value is a confident zero).  implicit=False: least
        squares over the stored entries only, targets a.  reg (finite, > 0) is the ridge on both tables; alpha is finite and >= 0.
        Each sweep solves every user's r x r normal equations against the item table, then every item's against the user table
        (tmf_gram_f32 + tmf_als_solve_rows_f32 on a GPU, torch.linalg.cholesky_ex in chunks of rows without one), and appends the
        objective both half-steps minimise to loss_history_ (teamoflow_amd/_als.py states it).
        solver='cg' (implicit's use_cg=True): every row takes ``cg_steps`` (1 - 32) conjugate-gradient steps from its current value
        instead of an exact solve (tmf_als_cg_rows_f32; teamoflow_amd/_als.py states the iteration) - several times fewer flops per
        sweep, n_components up to 256, and a sweep no longer minimises exactly, so expect a few sweeps more.
        Both sides must be exactly LinearEmbedding over indicator features (NotImplementedError otherwise), n_components <= 128
        (solver='cg': 256), float32 tables, one GPU, full batch; ``loss_graph``, ``lr`` and ``optimizer`` are not used.  The weights
        are drawn from user_weight_graph / item_weight_graph in the order ``fit`` draws them.  With solver='cholesky' only the item
        draw matters, because the first half-step solves the users exactly; with solver='cg' the user draw matters too: the first
        user half-step starts from it.  Leaves what ``fit`` leaves: user_embedding / item_embedding / *_trainable, so predict, the
        rankings, the metrics, similar_items / similar_users and save / load work as after ``fit``.  A row solve that meets a
        matrix that is not positive definite raises FloatingPointError after the last sweep.  Returns None."""
        reg, alpha = _als.check_hyper(reg, alpha)
        solver, cg_steps = _als.check_solver(solver, cg_steps)
        self._check_als_kernel('fit_als', solver)
        # full-batch on one GPU (or in torch without one): every other form is refused, and so is the L2 of fit() - ALS has reg
        self._answer('als', 'fit_als', also=('user_alpha', 'item_alpha'))
        if not (type(self.user_repr_graph) is LinearEmbedding and type(self.item_repr_graph) is LinearEmbedding
                and is_indicator(user_features) and is_indicator(item_features)):
            raise NotImplementedError('fit_als: both sides must be LinearEmbedding over indicator features (eye(n)); ALS on biased, '
                                      'ReLU or SparseFeatures sides is not built')
        n_users, n_user_features = user_features.shape
        n_items, n_item_features = item_features.shape
        U0 = self.user_weight_graph.initialize_weights(n_user_features, self.n_components)
        V0 = self.item_weight_graph.initialize_weights(n_item_features, self.n_components)
        interactions = _as_interactions(tf_interactions)
        if tuple(interactions.shape) != (n_users, n_items):
            raise ValueError(f'interactions of shape {tuple(interactions.shape)} for {n_users} users and {n_items} items')
        U, V = _als.fit(self, int(epochs), n_users, n_items, interactions, U0, V0, reg, alpha, bool(implicit), solver, cg_steps)
        self._reset_fit_products((False, False))
        self.item_bias_ = None              # ALS has no item term
        self.__dict__.pop('_state', None)   # an earlier engine fit's TrainState: its tables are not this model's any more
        self.user_embedding, self.item_embedding = U, V
        self.user_trainable, self.item_trainable = [U], [V]

    def _fold_in(self, side, interactions, reg, alpha, implicit, solver, cg_steps):
        name = ('users', 'items')[side]
        reg, alpha = _als.check_hyper(reg, alpha)
        solver, cg_steps = _als.check_solver(solver, cg_steps)
        self._check_als_kernel(f'fold_in_{name}', solver)   # a fold-in has no forms: ROUTES['als'] is about fit_als alone
        if self._item_sharded():
            raise NotImplementedError(f'item-row-sharded fit: this rank holds only its item rows; fold_in_{name} needs the whole table')
        table = getattr(self, ('item_embedding', 'user_embedding')[side], None)
        if table is None:
            raise ValueError(f'fold_in_{name}: the model has no fitted tables yet')
        return _als.fold_in(table, _as_interactions(interactions), reg, alpha, bool(implicit), solver, cg_steps)

    def fold_in_users(self, interactions, *, reg=0.01, alpha=1.0, implicit=True, solver='cholesky', cg_steps=3):
        """Extension (implicit's recalculate_user): the exact embeddings of users the fit has not seen, from their interactions with
        the fitted items.  interactions: SparseInteractions [n_new, n_items] whose ROWS are the new users.  -> float32 [n_new, r]:
        one ALS half-step (as fit_als, same reg / alpha / implicit meaning) against item_embedding, which a ``fit`` or a ``fit_als``
        may have trained (a bfloat16 table is upcast first).  The model is not modified.  The rows feed
        similar_users(queries=...) and _ops.predict_topk directly.  solver='cg': ``cg_steps`` conjugate-gradient steps from zeros
        instead of the exact solve (as fit_als).  n_components > 128 (solver='cg': 256): NotImplementedError."""
        return self._fold_in(0, interactions, reg, alpha, implicit, solver, cg_steps)

    def fold_in_items(self, interactions, *, reg=0.01, alpha=1.0, implicit=True, solver='cholesky', cg_steps=3):
        """fold_in_users for new items: interactions [n_new, n_users], rows = the new items, solved against user_embedding."""
        return self._fold_in(1, interactions, reg, alpha, implicit, solver, cg_steps)

    def _report(self, epoch, loss, seconds):
        if self.verbose and (epoch + 1) % 25 == 0:
            print(f'Epoch {epoch + 1} Complete | Loss {loss} | Runtime {seconds:.5} s')

    def _fit_sparse(self, epochs, n_users, n_items, interactions, lr, U0, V0, user_feat=None, item_feat=None):
        """Trains on the HIP engine and returns True; False (nothing trained) for a KLDivergenceLoss table with an empty class,
        which fit() hands to the generic path.  user_feat / item_feat: the SparseFeatures of a featured side (U0 / V0 are then its
        [n_features, r] weights)."""
        _lib.get()  # fail loudly here when the HIP engine cannot run
        self._sharded_epoch = None
        dev = default_device()
        t_plan = timeit.default_timer()
        if interactions.device != dev:
            interactions = interactions.to(dev)
        loss = _engine.loss_name(self.loss_graph)
        rec = _engine.LOSSES[loss]
        if rec.table and self.random_ind is None:
            raise SampleTableMissing(f'{type(self.loss_graph).__name__} needs generate_sample=True (random_ind is None)')
        form = self._engine_form()
        if form == 'batch_users':
            from .. import _minibatch
            _minibatch.fit_minibatch(self, epochs, n_users, n_items, interactions, lr, U0, V0, self.batch_users)
            return True
        if form != 'full':
            from .. import dist as tdist
            if form == 'shard_items':
                tdist.fit_item_sharded(self, epochs, n_users, n_items, interactions, lr, U0, V0, windows_per_rank=int(self.shard_items))
            else:
                tdist.fit_data_parallel(self, epochs, n_users, n_items, interactions, lr, U0, V0)
            return True
        st, c = self._sparse_state(loss, n_users, n_items, interactions, U0, V0, dev, user_feat, item_feat)
        if st is None:
            return False   # an empty class: no moments to take (the reference's arithmetic gives NaN; the generic path keeps that)
        denom = rec.denominator(st.plan)   # a loss over positives: their number; one that is a single scalar: its mean is itself
        self.loss_history_ = []
        step = self._sparse_step(st, loss, c, lr)
        # Launch-bound problems (a few hundred microseconds of kernels per epoch): capture an even number of
        # epochs into one hipGraph and replay it - the per-launch host cost disappears from the loop.
        G = min(epochs - epochs % 2, GRAPH_EPOCHS)
        use_graph = G >= 4 and rec.work(st.plan, st.wplan) <= GRAPH_MAX_WORK and os.environ.get('TMF_NO_GRAPH') is None \
            and self.optimizer != 'adam'
        every = self._resample_setting()[0]   # 0 for a loss that reads no table
        self.resample_rounds_ = int(rec.table)
        resample = None
        if every and epochs > every:   # more than one round: no graph (a captured graph holds the plan's pointers)
            use_graph = False

            def resample(j):   # round j's table into the live state; the tables, sides, moments and the interaction plan stay
                st.set_negatives(self._draw_round(j, n_items, n_users, dev))
        sums = self._run_epochs(step, epochs, G if use_graph else 0, denom, dev, t_plan, every, resample).cpu().numpy()
        self.loss_history_ = (sums / denom if denom else np.full(epochs, np.nan)).tolist()
        self._publish_sparse(st)
        return True

    def _sparse_state(self, loss, n_users, n_items, interactions, U0, V0, dev, user_feat=None, item_feat=None):
        """(TrainState, c) of a single-GPU full-batch fit, by the record of ``loss`` in _engine.LOSSES: the interaction plan, for the table
        family the checked negative table and its plan, prepared for the loss, c = the loss's parameter for this model, and the starting
        bias of a BiasedLinearEmbedding side.  (None, 0.0) for KL with an empty class."""
        rec = _engine.LOSSES[loss]
        plan = _engine.InteractionPlan(interactions.indices, interactions.values, n_users, n_items, **rec.plan_form())
        if rec.global_moments and (plan.n_pos == 0 or int((plan.val_u <= 0).sum()) == 0):
            return None, 0.0
        wplan = None
        biased = self._item_bias_setting()   # _route let it pass: a table loss.  WMRB then takes the sliced plan as the pair losses do
        if rec.table:
            R = _engine.checked_negatives(self.random_ind, n_users, n_items, dev)
            if getattr(self, '_sampling_weights', None) is not None:   # round 0 is drawn too; random_ind gave the shape
                R = self._draw_round(0, n_items, n_users, dev)
            wplan = _engine.wmrb_plan_for(plan, R, self.n_components, self.factor_dtype, force_sliced=rec.sliced_only or biased)
            rec.prepare(wplan, plan)   # before any epoch runs or is captured
            if getattr(self, 'sample_log_q_', None) is not None:   # the logQ offsets of this table: likewise, and noted on the plan
                wplan.slot_offsets(self.sample_log_q_.to(dev))
        r = self.n_components
        # a biased side starts from the bias an earlier fit left on the model, as in the reference (:139-146), else from zeros
        bias0 = [None if type(graph) is not BiasedLinearEmbedding else torch.zeros(r) if kept is None else kept
                 for graph, kept in ((self.user_repr_graph, self.user_linear_bias), (self.item_repr_graph, self.item_linear_bias))]
        # a ReLU side (only relu_engine lets one get here) carries its features itself; its hidden variables start from what an
        # earlier fit left on the model, else as get_repr draws them (:80-83): relu_weight ~ N(0, 1), relu_bias zeros
        relu0, feat = [None, None], [user_feat, item_feat]
        for side, (graph, rows, kept_w, kept_b) in enumerate((
                (self.user_repr_graph, n_users, self.user_relu_weight, self.user_relu_bias),
                (self.item_repr_graph, n_items, self.item_relu_weight, self.item_relu_bias))):
            if type(graph) is ReLUEmbedding:
                aux, n_features = 5 * r, rows if feat[side] is None else int(feat[side].shape[1])
                relu0[side] = dict(F=feat[side],
                                   Wr0=torch.randn(n_features, aux, device=dev) if kept_w is None else kept_w,
                                   b0=torch.zeros(aux, device=dev) if kept_b is None else kept_b)
                feat[side] = None
        st = _engine.TrainState(U0, V0, plan, r, wplan, dtype=self.factor_dtype, user_bias=bias0[0], item_bias=bias0[1],
                                user_feat=feat[0], item_feat=feat[1], user_relu=relu0[0], item_relu=relu0[1],
                                **({rec.flag: True} if rec.flag else {}),
                                **({'item_scalar_bias': torch.zeros(n_items, device=dev)} if biased else {}))
        alphas = self._alphas()
        if any(alphas):   # never called with zeros: an unpenalised fit is today's state, launch for launch
            st.set_l2(*alphas)
        if self._correction_setting() == 'logq' and wplan is not None and wplan.off is None:
            return st, _engine.catalog_ratio(self)   # uniform tables: l is the constant log(S / n_items) - catalog_scale's c, its kernel
        return st, rec.param(self)

    def _sparse_step(self, st, loss, c, lr):
        """step(epoch, out): one epoch, its loss sum into ``out``, by the reference's fresh Adam or by optimizer='adam' (kept moments)."""
        adam = _engine.adam_constants(lr)
        if self.optimizer not in ('fresh_adam', 'adam'):
            raise ValueError(f"optimizer={self.optimizer!r}: 'fresh_adam' (the reference's behaviour) or 'adam'")
        if self.optimizer == 'fresh_adam':
            return lambda epoch, out: _engine.epoch_sides(st, adam, out, loss, c)
        if self.factor_dtype is not torch.float32:
            raise ValueError("optimizer='adam' (persistent moments) needs float32 factor tables")
        lib = _lib.get()
        # a penalised side has its gradient table already (TrainState.set_l2); only plain sides get here
        gU, gV = (torch.empty_like(W) if side is None else side.G for W, side in zip((st.U, st.V), st.sides))
        sides = [(W, G, torch.zeros_like(W), torch.zeros_like(W), l2)
                 for W, G, l2 in ((st.U, gU, st.l2[0]), (st.V, gV, st.l2[1]))]   # table, gradient, m, v, l2 = 2 alpha
        if st.ib is not None:   # the scalar item bias, moments of its own, never penalised: the vector as a [rows, 4] table
            st.ib.epi = _lib.EPI_GRAD   # its second buffer receives the raw gradient; b is stepped in place below
            b4, g4 = st.ib.b.view(-1, 4), st.ib.b_nxt.view(-1, 4)
            sides.append((b4, g4, torch.zeros_like(b4), torch.zeros_like(b4), 0.0))

        def persistent(epoch, out):   # raw gradients of both sides from the pre-update tables, then one Adam step with state, in place
            a = lib.tmf_adam_step(float(lr), epoch + 1)
            _engine.run_epoch(st, a, out, loss, c, _lib.EPI_GRAD, gV, None, _lib.EPI_GRAD, gU)
            for W, G, M, V2, l2 in sides:
                width = 4 if st.ib is not None and W is sides[-1][0] else self.n_components
                if l2:   # the moments see g' = g + l2 w
                    _lib.check(lib.tmf_adam_state_rows_l2_f32(W, G, M, V2, W.shape[0],
                                                              self.n_components, a, l2, _lib.stream_ptr()), lib)
                    continue
                _lib.check(lib.tmf_adam_state_rows_f32(W, G, M, V2, W.shape[0],
                                                       width, a, _lib.stream_ptr()), lib)
        return persistent

    def _run_epochs(self, step, epochs, G, denom, dev, t_plan, every=0, resample=None):
        """step(epoch, out) for every epoch (G > 0: replays of one hipGraph of G epochs, then the rest), reports and timings.  -> loss sums.
        resample (with G = 0): resample(j) is called before the first epoch of every round j = epoch // every >= 1, between synchronisations;
        its time goes to resample_seconds_ (and, like everything in the loop, to fit_seconds_)."""
        loss_sums = torch.zeros(max(epochs, 1), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        t0 = timeit.default_timer()
        self.plan_seconds_ = t0 - t_plan  # extension: index structures + table set-up of this fit (once, not per epoch)
        done = 0
        if G:
            block = torch.zeros(G, dtype=torch.float64, device=dev)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for e in range(G):
                    step(e, block[e:e + 1])
            # capture only records; the tables are still the initial ones (G is even: buffers line up again)
            t_prev = timeit.default_timer() - t0
            while done + G <= epochs:
                graph.replay()
                loss_sums[done:done + G].copy_(block)
                done += G
                self.graph_epochs_ = done
                if self.verbose and denom:
                    t_now = None
                    for e in range(done - G, done):
                        if (e + 1) % 25 == 0:
                            if t_now is None:
                                float(loss_sums[e])  # syncs: the replay has finished
                                t_now = timeit.default_timer() - t0
                            # cumulative runtime at epoch e, interpolated inside this replay
                            self._report(e, float(loss_sums[e]) / denom, t_prev + (t_now - t_prev) * (e + 1 - (done - G)) / G)
                    if t_now is not None:
                        t_prev = t_now
        for epoch in range(done, epochs):
            if resample is not None and epoch and epoch % every == 0:
                torch.cuda.synchronize(dev)
                t_draw = timeit.default_timer()
                resample(epoch // every)
                torch.cuda.synchronize(dev)
                self.resample_seconds_ += timeit.default_timer() - t_draw
                self.resample_rounds_ += 1
            step(epoch, loss_sums[epoch:epoch + 1])
            if self.verbose and (epoch + 1) % 25 == 0:
                loss = float(loss_sums[epoch]) / denom if denom else float('nan')  # syncs
                self._report(epoch, loss, timeit.default_timer() - t0)
        torch.cuda.synchronize(dev)
        self.fit_seconds_ = timeit.default_timer() - t0
        return loss_sums[:epochs]

    def _publish_sparse(self, st):
        """What a fit leaves on the model: the tables, and for a biased side what _fit_generic leaves - [weights, bias], the [1, r]
        bias kept on the model, a leaf that requires grad because a later generic fit differentiates with respect to it."""
        r = self.n_components
        self._state = st
        self.user_embedding, self.item_embedding = st.U[:, :r], st.V[:, :r]
        self.user_trainable, self.item_trainable = [self.user_embedding], [self.item_embedding]
        self.item_bias_ = None if st.ib is None else st.ib.value
        if st.bias_u is not None:
            self.user_linear_bias = st.bias_u.b[:r].clone().view(1, r).requires_grad_(True)
            self.user_trainable = [st.bias_u.W[:, :r], self.user_linear_bias]
        if st.bias_v is not None:
            self.item_linear_bias = st.bias_v.b[:r].clone().view(1, r).requires_grad_(True)
            self.item_trainable = [st.bias_v.W[:, :r], self.item_linear_bias]
        # a side over SparseFeatures: the embedding is E = F W, the variable its weights W [n_features, r]
        if st.feat_u is not None:
            self._feature_weights[0], self.user_trainable = st.feat_u.W, [st.feat_u.W[:, :r]]
        if st.feat_v is not None:
            self._feature_weights[1], self.item_trainable = st.feat_v.W, [st.feat_v.W[:, :r]]
        # a ReLU side: [weights [aux, r], relu_weight [n_features, aux], relu_bias [1, aux]], the two hidden variables kept on the
        # model as leaves that require grad (relu_weight a view of the engine's padded table: it is as large as the features)
        for side, relu in enumerate((st.relu_u, st.relu_v)):
            if relu is not None:
                self._relu_sides[side] = relu
                kept_w = relu.Wr[:, :relu.aux].detach().requires_grad_(True)
                kept_b = relu.b[:relu.aux].clone().view(1, relu.aux).requires_grad_(True)
                trainable = [relu.W[:, :r], kept_w, kept_b]
                if side == 0:
                    self.user_relu_weight, self.user_relu_bias, self.user_trainable = kept_w, kept_b, trainable
                else:
                    self.item_relu_weight, self.item_relu_bias, self.item_trainable = kept_w, kept_b, trainable

    def _fit_generic(self, epochs, user_features, item_features, interactions, lr, U, V):
        """The reference's dense loop (:128-187) over arbitrary plug-ins, differentiated by autograd."""
        self._sharded_epoch = None
        dev = U.device
        interactions = interactions.to(dev)
        idx = interactions.indices
        alpha, omb1, omb2, eps = (float(x) for x in _adam_scalars(lr))
        self.loss_history_ = []
        cumulative_time = 0.0
        random_ind = None if self.random_ind is None else torch.as_tensor(self.random_ind).to(dev)
        user_alpha, item_alpha = self._alphas()
        every = self._resample_setting()[0]
        self.resample_rounds_ = int(isinstance(self.loss_graph, TABLE_LOSSES) and random_ind is not None)
        feeds = next((feeds for feeds, classes in _FEEDS.items() if isinstance(self.loss_graph, classes)), 'dense')   # Loss.feeds
        if random_ind is not None and getattr(self, '_sampling_weights', None) is not None:   # popularity: round 0 is drawn too
            random_ind = self._draw_round(0, item_features.shape[0], user_features.shape[0], dev)
        # scalar_item_bias: one more leaf, from zeros, stepped with the other variables and never penalised
        bias = torch.zeros(item_features.shape[0], dtype=torch.float32, device=dev, requires_grad=True) if self._item_bias_setting() else None
        # sampling_correction='logq' (SampledSoftmaxLoss and its subclasses; _route refused the rest): l[R] off the sampled scores of
        # the round's table; under uniform tables l is the constant log(S / n_items), which is the loss's own catalog_scale
        loss_graph, ell = self.loss_graph, getattr(self, 'sample_log_q_', None)
        ell = None if ell is None else ell.to(dev)
        if self._correction_setting() == 'logq' and ell is None:
            loss_graph = copy.copy(loss_graph)
            loss_graph.catalog_scale = True
        for epoch in range(epochs):
            start = timeit.default_timer()
            if every and epoch and epoch % every == 0 and random_ind is not None:   # round epoch // every: its own table, random_ind stays
                random_ind = self._draw_round(epoch // every, item_features.shape[0], user_features.shape[0], dev)
                if dev.type == 'cuda':
                    torch.cuda.synchronize(dev)
                self.resample_seconds_ += timeit.default_timer() - start
                self.resample_rounds_ += 1
            user_embedding, self.user_trainable = self.user_repr_graph.get_repr(
                features=user_features, weights=U, relu_weight=self.user_relu_weight, relu_bias=self.user_relu_bias,
                linear_bias=self.user_linear_bias)
            item_embedding, self.item_trainable = self.item_repr_graph.get_repr(
                features=item_features, weights=V, relu_weight=self.item_relu_weight, relu_bias=self.item_relu_bias,
                linear_bias=self.item_linear_bias)
            self._keep_aux_variables()
            predictions = user_embedding @ item_embedding.T
            if bias is not None:
                predictions = predictions + bias[None, :]
            tf_sample_predictions = tf_prediction_serial = None
            if feeds == 'samples':
                if random_ind is None:
                    raise SampleTableMissing(f'{type(self.loss_graph).__name__} needs generate_sample=True (random_ind is None)')
                tf_sample_predictions = torch.gather(predictions, 1, random_ind.to(torch.int64))
                if ell is not None:
                    tf_sample_predictions = tf_sample_predictions - ell[random_ind.to(torch.int64)]
            if feeds != 'dense':
                tf_prediction_serial = predictions[idx[:, 0], idx[:, 1]]
                predictions = None
            loss_fn = loss_graph.get_loss(tf_interactions=interactions, tf_sample_predictions=tf_sample_predictions,
                                          tf_prediction_serial=tf_prediction_serial, predictions=predictions,
                                          n_items=self.n_items, n_samples=self.n_samples)
            variables = self.user_trainable + self.item_trainable + ([] if bias is None else [bias])
            objective = loss_fn.sum()
            for penalty, graph, trainable in ((user_alpha, self.user_repr_graph, self.user_trainable),
                                              (item_alpha, self.item_repr_graph, self.item_trainable)):
                if penalty:   # penalty ||W||_F^2 over the side's weight matrices: the weights, and relu_weight of a ReLU side - never a bias
                    for w in trainable[:2 if isinstance(graph, ReLUEmbedding) else 1]:
                        objective = objective + penalty * (w * w).sum()
            grads = torch.autograd.grad(objective, variables, allow_unused=True)
            with torch.no_grad():
                for w, g in zip(variables, grads):
                    if g is not None:  # fresh Adam, t = 1 (:176)
                        w -= ((g * omb1) * alpha) / (torch.sqrt((g * g) * omb2) + eps)
            cumulative_time += timeit.default_timer() - start
            loss_one_epoch = float(loss_fn.detach().mean())
            self.loss_history_.append(loss_one_epoch)
            self._report(epoch, loss_one_epoch, cumulative_time)
        self.fit_seconds_ = cumulative_time
        if bias is not None:
            self.item_bias_ = bias.detach()
        with torch.no_grad():
            self.user_embedding, self.user_trainable = self.user_repr_graph.get_repr(
                features=user_features, weights=U, relu_weight=self.user_relu_weight, relu_bias=self.user_relu_bias,
                linear_bias=self.user_linear_bias)
            self.item_embedding, self.item_trainable = self.item_repr_graph.get_repr(
                features=item_features, weights=V, relu_weight=self.item_relu_weight, relu_bias=self.item_relu_bias,
                linear_bias=self.item_linear_bias)

    def _keep_aux_variables(self):
        if isinstance(self.user_repr_graph, BiasedLinearEmbedding):
            _, self.user_linear_bias = self.user_trainable
        if isinstance(self.user_repr_graph, ReLUEmbedding):
            _, self.user_relu_weight, self.user_relu_bias = self.user_trainable
        if isinstance(self.item_repr_graph, BiasedLinearEmbedding):
            _, self.item_linear_bias = self.item_trainable
        if isinstance(self.item_repr_graph, ReLUEmbedding):
            _, self.item_relu_weight, self.item_relu_bias = self.item_trainable

    # ------------------------------------------------------------------------------------------
    # cold start: embeddings of rows the fit has not seen, from their features
    # ------------------------------------------------------------------------------------------
    def _embed(self, side, features):
        name = ('user', 'item')[side]
        if not getattr(self, '_sparse_feature_sides', (False, False))[side]:
            raise ValueError(f'embed_{name}s: the {name} side of the last fit was not trained over SparseFeatures (there are no feature '
                             f'weights to multiply)')
        if not isinstance(features, SparseFeatures):
            raise TypeError(f'embed_{name}s takes SparseFeatures')
        graph = (self.user_repr_graph, self.item_repr_graph)[side]
        trainable = (self.user_trainable, self.item_trainable)[side]
        relu = getattr(self, '_relu_sides', (None, None))[side]
        W = trainable[0].detach()
        n_features = W.shape[0] if relu is None else relu.n_features
        if features.shape[1] != n_features:
            raise ValueError(f'embed_{name}s: features of {features.shape[1]} columns for weights of {n_features} features')
        if relu is not None:     # an engine fit of a ReLU side: the two forward kernels on the variables it left
            return _engine.embed_relu(features, relu)[:, :self.n_components]
        padded = self._feature_weights[side]
        if padded is not None:   # an engine fit: the forward kernel on the padded weights it left
            return _engine.embed_features(features, padded, self.n_components)[:, :self.n_components]
        aux = ((self.user_relu_weight, self.user_relu_bias, self.user_linear_bias),
               (self.item_relu_weight, self.item_relu_bias, self.item_linear_bias))[side]
        with torch.no_grad():   # a generic fit: the plug-in's own definition over the dense rows
            return graph.get_repr(features=features.to_dense(W.device), weights=W, relu_weight=aux[0], relu_bias=aux[1],
                                  linear_bias=aux[2])[0]

    def embed_users(self, features):
        """Extension: F_new W_u [rows, r] for the trained user weights - the embeddings of users the fit has not seen, from their
        feature rows (SparseFeatures with the training matrix's columns).  Needs a user side trained over SparseFeatures."""
        return self._embed(0, features)

    def embed_items(self, features):
        """Extension: F_new W_i [rows, r] for the trained item weights (embed_users for the item side)."""
        return self._embed(1, features)

    # ------------------------------------------------------------------------------------------
    # prediction and ranking
    # ------------------------------------------------------------------------------------------
    def predict(self, A=None):
        """:189-201.  All scores [n_users, n_items]; with A also the scores where A == 0 (row-major)."""
        if self._item_sharded():
            raise NotImplementedError('item-row-sharded fit: this rank holds only its item rows, the dense [n_users, n_items] score '
                                      'matrix is not available; recall_at_k / precision_at_k / retrieve_user_recs rank over the '
                                      'windows (dist.sharded_top_items), dist.gather_item_embedding assembles the table where it fits')
        U, V, _ = self._score_tables()
        all_predictions = _ops.predict_gemm(U, V)
        if A is not None:
            A = torch.as_tensor(A).to(all_predictions.device)
            return all_predictions, all_predictions[A == 0]
        return all_predictions

    def predict_ranks(self, A):
        """:203-216.  Global descending ranking of the flattened unobserved predictions."""
        _, unobserved = self.predict(A)
        return torch.sort(unobserved, descending=True, stable=True)[1]

    def _score_tables(self):
        """(U, V, fused) every score and ranking of this model is formed from: the embeddings, or with a trained scalar item bias
        (item_bias_) the augmented tables [U | 1], [V | b] (augmented_tables), whose product is U V^T + b.  fused: the width fits the
        fused ranking kernels (always, without a bias: the calls decide by the width as before)."""
        b = getattr(self, 'item_bias_', None)
        if b is None:
            return self.user_embedding, self.item_embedding, True
        return augmented_tables(self.user_embedding, self.item_embedding, b)

    def _user_blocks(self):
        m, n = self.user_embedding.shape[0], self.item_embedding.shape[0]
        rows = max(1, min(m, PREDICT_CHUNK_BYTES // (4 * max(n, 1))))
        return [(b, min(b + rows, m)) for b in range(0, m, rows)]

    def _item_sharded(self):
        """An item-row-sharded fit over several ranks: item_embedding holds only this rank's rows."""
        ep = getattr(self, '_sharded_epoch', None)
        return ep is not None and ep.world > 1

    def _exclusion(self, exclude):
        """exclude (SparseInteractions, a dense table or an _ops.Exclusion; rows = this model's users) as a device CSR."""
        n_items = self._n_items_fit if self._item_sharded() else self.item_embedding.shape[0]
        return _ops.build_exclusion(exclude, self.user_embedding.shape[0], n_items, device=self.user_embedding.device)

    def _top_items(self, k, clamp, users=None, exclude=None):
        """Top-k item ids (int32) for every user, scored block by block: the [m, n] matrix is only
        ever materialised one block of users at a time.  exclude: pairs left out of the ranking (-1 past a user's
        eligible items)."""
        ex = None if exclude is None else self._exclusion(exclude)
        if self._item_sharded():
            # item_embedding holds only this rank's rows - rank over the windows (a collective)
            from .. import dist as tdist
            top = tdist.sharded_top_items(self, k, clamp, users=users, exclude=ex)
            return top[0] if users is not None else top

        U, V, fused = self._score_tables()   # with a scalar item bias [U | 1], [V | b]

        def ranked(b, e):   # users [b, e) through their block of scores; the exclusion is written into the block
            scores = _ops.predict_gemm(U[b:e], V)
            return _ops.topk_stable(scores, k, clamp_negatives=clamp, exclude=None if ex is None else ex.shifted(b), overwrite=True)

        if users is not None:
            return ranked(users, users + 1)[0]
        if fused and _ops.fused_topk_supported(U, V, k):
            return _ops.predict_topk(U, V, k, clamp_negatives=clamp,
                                     arithmetic=getattr(self, 'predict_arithmetic', None), exclude=ex)
        out = [ranked(b, e) for b, e in self._user_blocks()]
        return torch.cat(out) if len(out) > 1 else out[0]

    def _hits_and_relevant(self, A, k, exclude=None):
        """hits[u] = #top-k items with a non-zero entry in A, relevant[u] = #entries of A > 0
        (:245-254).  A: dense [m, n] tensor, or SparseInteractions (extension for shapes whose dense
        table does not fit).  With exclude the lists may end in -1 (fewer eligible items than k): those slots are never hits."""
        top = self._top_items(k, clamp=True, exclude=exclude)
        valid = None
        if exclude is not None:
            valid = top >= 0
            top = torch.where(valid, top, torch.zeros_like(top))   # a gatherable id in the fill slots, masked out below
        top = top.to(torch.int64)
        if isinstance(A, SparseInteractions):
            A = A.to(top.device)
            m, n = A.dense_shape
            nz = A.values != 0
            # column first, mask second (see _ops._decode_table)
            keys = A.indices[:, 0][nz] * n + A.indices[:, 1][nz]
            if keys.numel() > 1 and not bool((keys[1:] >= keys[:-1]).all()):   # row-major input (the reference's format) is sorted already
                keys = torch.sort(keys)[0]
            q = (torch.arange(m, device=top.device)[:, None] * n + top).reshape(-1)
            pos = torch.clamp(torch.searchsorted(keys, q), max=max(keys.numel() - 1, 0))
            found = (keys[pos] == q).reshape(top.shape) if keys.numel() else torch.zeros_like(top, dtype=torch.bool)
            relevant = torch.bincount(A.indices[:, 0][A.values > 0], minlength=m).to(torch.float32)
        else:
            A = torch.as_tensor(A).to(device=top.device, dtype=torch.float32)
            found = gather_matrix_indices(A, top) != 0
            relevant = torch.count_nonzero(A > 0.0, dim=1).to(torch.float32)
        if valid is not None:
            found = found & valid
        return found.sum(dim=1).to(torch.float32), relevant

    def recall_at_k(self, A, k=10, preserve_rows=False, *, exclude=None):
        """:218-269.  Per-user hits@k / #positives; the caller takes the mean.  exclude (extension, LightFM's
        train_interactions): (user, item) pairs left out of the ranking - SparseInteractions or a dense table."""
        hits, relevant = self._hits_and_relevant(A, k, exclude=exclude)
        if not preserve_rows:
            mask = relevant != 0.0
            return hits[mask] / relevant[mask]
        recall = hits / relevant
        return torch.where(torch.isnan(recall), torch.zeros_like(recall), recall)

    def precision_at_k(self, A, k=10, preserve_rows=False, *, exclude=None):
        """:271-304.  exclude: as recall_at_k."""
        hits, relevant = self._hits_and_relevant(A, k, exclude=exclude)
        if not preserve_rows:
            return hits[relevant != 0.0] / k
        return hits / k

    def f1_at_k(self, A, k=10, beta=1.0, *, exclude=None):
        """:306-318 (the reference's formula, denominator beta^2 (p + r)).  exclude: as recall_at_k."""
        if exclude is not None:
            exclude = self._exclusion(exclude)   # built once for both rankings
        prec = self.precision_at_k(A, k=k, exclude=exclude).mean()
        rec = self.recall_at_k(A, k=k, exclude=exclude).mean()
        return ((1 + beta ** 2) * prec * rec) / (beta ** 2 * (prec + rec))

    def _dcg_terms(self, dense_interactions):
        predictions = self.predict()
        m, n = predictions.shape
        ranks = _ops.topk_stable(predictions, n).to(torch.int64)
        A = torch.as_tensor(dense_interactions).to(device=predictions.device, dtype=torch.float32)
        numerator = torch.pow(2.0, gather_matrix_indices(A, ranks)) - 1.0
        order = torch.arange(1, n + 1, dtype=torch.float32, device=predictions.device)
        denominator = torch.log1p(order) / float(np.log(np.float32(2.0)))
        return numerator, denominator

    @staticmethod
    def _sparse_dcg_path(A, exclude):
        """Sparse test tables and exclude= take the top-k + tmf_dcg_idcg_f32 path; a dense table without exclude keeps the reference's
        full sort (_dcg_terms)."""
        return exclude is not None or (not torch.is_tensor(A) and hasattr(A, 'indices') and hasattr(A, 'values'))

    def _dcg_setup(self, A, k, exclude):
        """(graded test table, effective k, exclusion or None, zero gains per user or None) of the sparse DCG path, every argument
        checked before anything is launched."""
        if self._item_sharded():
            raise NotImplementedError('item-row-sharded fit: this rank holds only its item rows; dcg / idcg / ndcg need every window '
                                      '(dist.gather_item_embedding assembles the table where it fits)')
        k = int(k)
        if k < 1:
            raise ValueError(f'k={k} must be >= 1')
        m, n = self.user_embedding.shape[0], self.item_embedding.shape[0]
        table = _ops.graded_csr(A, m, n, device=self.user_embedding.device)
        ex, n_zero = None, None
        if exclude is not None:
            ex = self._exclusion(exclude)
            both = _ops.overlap_count(table, ex, m, n)
            if both:
                raise ValueError(f'{both} (user, item) pairs are both test entries and excluded: an excluded item cannot be retrieved, '
                                 f'so it cannot count in the ideal ranking')
            if ex.user_base == 0 and ex.item_base == 0 and ex.n_items == n:   # a whole table (build_exclusion): distinct ids < n
                excluded = ex.rowptr[1:m + 1] - ex.rowptr[:m]
            else:
                excluded = _ops.exclusion_counts(ex, m, n)
            n_zero = n - excluded.to(table.rowptr.device) - table.stored()
        return table, min(k, n), ex, n_zero

    def _dcg_idcg(self, A, k, exclude, want_dcg, want_idcg):
        table, k, ex, n_zero = self._dcg_setup(A, k, exclude)
        top = self._top_items(k, clamp=False, exclude=ex) if want_dcg else None
        dcg, idcg = _ops.dcg_idcg(table, top, k, n_zero=n_zero, want_dcg=want_dcg, want_idcg=want_idcg)
        return dcg, idcg, table

    def dcg_at_k(self, dense_interactions, k=10, *, exclude=None):
        """:320-351.  Extension: a SparseInteractions table and exclude (as recall_at_k) rank the top-k of the fused kernels (raw
        scores, exclude= left out; retrieve_user_recs' lists) and look up the gains 2^a - 1 of the listed items in the test table's
        CSR (tmf_dcg_idcg_f32) - no [m, n] scores.  A dense table without exclude keeps the reference's full sort."""
        if self._sparse_dcg_path(dense_interactions, exclude):
            return self._dcg_idcg(dense_interactions, k, exclude, True, False)[0]
        numerator, denominator = self._dcg_terms(dense_interactions)
        return (numerator / denominator[None, :])[:, :k].sum(dim=1)

    def idcg_at_k(self, dense_interactions, k=10, *, exclude=None):
        """:353-384.  Extension (sparse table or exclude, as dcg_at_k): the k largest gains of the user's row, padded with the zero
        gains of the eligible items the row does not store - independent of the model, no GEMM."""
        if self._sparse_dcg_path(dense_interactions, exclude):
            return self._dcg_idcg(dense_interactions, k, exclude, False, True)[1]
        numerator, denominator = self._dcg_terms(dense_interactions)
        ideal = torch.sort(numerator, dim=1, descending=True, stable=True)[0]
        return (ideal / denominator[None, :])[:, :k].sum(dim=1)

    def ndcg_at_k(self, A, k=10, preserve_rows=False, *, exclude=None):
        """:386-413.  Extension (sparse A or exclude, as dcg_at_k): one top-k and one launch for DCG and IDCG.  A pair that is both a
        test entry and excluded raises ValueError."""
        if self._sparse_dcg_path(A, exclude):
            dcg, idcg, table = self._dcg_idcg(A, k, exclude, True, True)
            ndcg = dcg / idcg
            if not preserve_rows:
                return ndcg[table.stored().to(ndcg.device) > 0]
            return torch.where(~torch.isnan(ndcg), ndcg, torch.zeros_like(ndcg))
        ndcg = self.dcg_at_k(A, k) / self.idcg_at_k(A, k)
        if not preserve_rows:
            A = torch.as_tensor(A).to(ndcg.device)
            return ndcg[torch.count_nonzero(A, dim=1) > 0]
        return torch.where(~torch.isnan(ndcg), ndcg, torch.zeros_like(ndcg))

    def _rank_pairs(self, A, exclude):
        """(positives' CSR rowptr, cols, int32 ranks, exclusion CSR or None) of item_ranks."""
        if self._item_sharded():
            raise NotImplementedError('item-row-sharded fit: this rank holds only its item rows; full-catalog ranks need every '
                                      'window (dist.gather_item_embedding assembles the table where it fits)')
        ex = None if exclude is None else self._exclusion(exclude)
        U, V, fused = self._score_tables()
        arithmetic = getattr(self, 'predict_arithmetic', None)
        if not fused and arithmetic == 'split':   # a bias made the width 257: the block form, which 'auto' and 'fp32' take by themselves
            arithmetic = 'fp32'
        rowptr, cols, ranks = _ops.item_ranks(U, V, A, exclude=ex, arithmetic=arithmetic, return_pairs=True)
        return rowptr, cols, ranks, ex

    def item_ranks(self, A, *, exclude=None):
        """Extension (LightFM's predict_rank): the full-catalog rank of every held-out positive, without the [m, n] scores.
        A: SparseInteractions or a dense table; its entries > 0 are the positives (recall_at_k's "relevant"; duplicates count
        once).  rank(u, i) = the number of eligible items j != i - not in ``exclude`` (LightFM's train_interactions); the other
        positives count - that score above i, equal scores ordered by ascending id (retrieve_user_recs' order), so 0 is the top
        and rank < k exactly when i is in retrieve_user_recs(k=k, exclude=exclude)[u] (fp32 and split arithmetic).  Scores are the
        raw u.v (no clamp); a NaN score is never counted above anyone.  A pair both positive and excluded raises ValueError.
        Returns (indices [P, 2] int64 (user, item), row-major ascending; ranks [P] int64), on the model's device."""
        rowptr, cols, ranks, _ = self._rank_pairs(A, exclude)
        P = ranks.numel()
        users = _ops._csr_rows(rowptr)
        return torch.stack([users, cols[:P].to(torch.int64)], 1), ranks.to(torch.int64)

    def _per_user(self, value, counts, preserve_rows):
        if not preserve_rows:
            return value[counts > 0]
        return torch.where(counts > 0, value, torch.zeros_like(value))

    def auc_score(self, A, preserve_rows=False, *, exclude=None):
        """Extension (LightFM's auc_score): per-user AUC of the held-out positives against the eligible negatives, from
        item_ranks (same arguments); the caller takes the mean.  With P positives and N = n_items - |excluded| - P negatives and the
        ranks sorted r_0 < ... < r_{P-1}, r_t - t negatives score above the t-th positive: AUC = 1 - sum_t (r_t - t) / (P N), in
        fp64, returned as float32; 1.0 when N = 0.  Users without positives are dropped, or get 0 with preserve_rows
        (recall_at_k's convention)."""
        rowptr, _, ranks, ex = self._rank_pairs(A, exclude)
        m, n = rowptr.numel() - 1, self.item_embedding.shape[0]
        auc, counts = _ops.auc_from_ranks(rowptr, ranks, n, _ops.exclusion_counts(ex, m, n) if ex is not None else None)
        return self._per_user(auc, counts, preserve_rows)

    def reciprocal_rank(self, A, preserve_rows=False, *, exclude=None):
        """Extension (LightFM's reciprocal_rank): per user 1 / (1 + the best rank of a held-out positive), from item_ranks (same
        arguments); float32, the caller takes the mean.  Users without positives as in auc_score."""
        rowptr, _, ranks, _ = self._rank_pairs(A, exclude)
        rr, counts = _ops.reciprocal_rank_from_ranks(rowptr, ranks, self.item_embedding.shape[0])
        return self._per_user(rr, counts, preserve_rows)

    def retrieve_user_recs(self, user=None, k=None, *, exclude=None):
        """:416-438.  Item ids ranked by score (numpy int32, like tf.math.top_k(...).indices.numpy()).  exclude (extension):
        (user, item) pairs left out - SparseInteractions or a dense table over all users (also with `user`); slots past a
        user's eligible items hold -1."""
        num_items = self.item_embedding.shape[0]
        kk = num_items if k is None else k
        return self._top_items(kk, clamp=False, users=user, exclude=exclude).cpu().numpy()

    def _similar(self, side, rows, k, metric, include_self, queries):
        name = ('user', 'item')[side]
        if self._item_sharded():
            raise NotImplementedError(f'item-row-sharded fit: this rank holds only its item rows; similar_{name}s needs the whole '
                                      f'table (dist.gather_item_embedding assembles it where it fits)')
        table = (self.user_embedding, self.item_embedding)[side]
        single = isinstance(rows, (int, np.integer)) and not isinstance(rows, bool)
        idx, vals = _ops.similar_rows(table, k, ids=[rows] if single else rows, queries=queries, metric=metric,
                                      include_self=include_self, arithmetic=getattr(self, 'predict_arithmetic', None),
                                      block_bytes=PREDICT_CHUNK_BYTES)
        idx, vals = idx.cpu().numpy(), vals.cpu().numpy()
        return (idx[0], vals[0]) if single else (idx, vals)

    def similar_items(self, items=None, k=10, *, metric='cosine', include_self=False, queries=None):
        """Extension (implicit's similar_items): the k items nearest to each query item by their trained embeddings, without an
        [n, n] matrix -> (ids int32, similarities float32) as NumPy arrays, similarity descending, ties by ascending id.
        items: None = every item, an int = one item (1-D results, as retrieve_user_recs(user=...)), or a sequence / array / tensor
        of ids, in any order and with repeats ([q, k] results).  An item never returns itself unless include_self is set.
        queries: [q, r] embeddings instead of ids - for instance embed_items(SparseFeatures(...)) of items the fit has not seen;
        nothing is excluded then.  metric: 'cosine' (unit rows from tmf_unit_rows_*: right for rows of any scale, a zero row has
        similarity 0 with everything) or 'dot'.  Ranked under predict_arithmetic; fp32 and bf16 stored tables.
        k outside [1, n - 1] ([1, n] when nothing is excluded), a bad metric, ids together with queries or queries of another
        width raise ValueError, an id out of range IndexError - all before the engine is touched."""
        return self._similar(1, items, k, metric, include_self, queries)

    def similar_users(self, users=None, k=10, *, metric='cosine', include_self=False, queries=None):
        """Extension (implicit's similar_users): similar_items over user_embedding."""
        return self._similar(0, users, k, metric, include_self, queries)

    # ------------------------------------------------------------------------------------------
    # persistence
    # ------------------------------------------------------------------------------------------
    def save_model(self):
        """:440-462.  (config dict with the reference's display keys, results dict)."""
        dict_config = {'Latent Dimension': self.n_components, 'User Embedding': self.user_repr_graph,
                       'Item Embedding': self.item_repr_graph, 'Loss': self.loss_graph,
                       'User Initialization': self.user_weight_graph, 'Item Initialization': self.item_weight_graph,
                       'Number of Users': self.n_users, 'Number of Items': self.n_items,
                       'Number of Samples': self.n_samples, 'Generate Sample': self.generate_sample}
        dict_results = {'User Embedding': self.user_embedding, 'Item Embedding': self.item_embedding,
                        'User Variables': self.user_trainable, 'Item Variables': self.item_trainable}
        return dict_config, dict_results

    _DISPLAY_KEYS = {'Latent Dimension': 'n_components', 'User Embedding': 'user_repr_graph',
                     'Item Embedding': 'item_repr_graph', 'Loss': 'loss_graph',
                     'User Initialization': 'user_weight_graph', 'Item Initialization': 'item_weight_graph',
                     'Number of Users': 'n_users', 'Number of Items': 'n_items', 'Number of Samples': 'n_samples',
                     'Generate Sample': 'generate_sample'}

    def save(self, path, include_samples=True, allow_pickle=False):
        """Extension: save_model()'s two dicts plus the tables in ONE file (torch.save).  The built-in
        plug-ins are stored as plain data (class name + constructor state), so the file loads with
        ``torch.load(weights_only=True)``; a user-defined plug-in object can only be stored pickled
        (``allow_pickle=True`` here AND in ``load``).  ``include_samples=False`` leaves the [m, S] negative table out."""
        if self._item_sharded():
            raise ValueError('item-row-sharded model: this rank holds users %s and %d of the item rows only - assemble the tables '
                             'first (dist.gather_user_embedding / gather_item_embedding) or save one file per rank from them'
                             % (self.user_block, int(self.item_rows.numel())))
        _save_to_disk(self, path, include_samples, allow_pickle)

    @classmethod
    def load(cls, path, device=None, allow_pickle=False):
        """Inverse of ``save``: a model ready for predict / recall_at_k / a further fit.  ``allow_pickle=True`` unpickles
        arbitrary objects from the file - only for files you wrote yourself."""
        return _load_from_disk(cls, path, device, allow_pickle)

    @classmethod
    def from_saved(cls, config):
        """:465-475: ``cls(**config)``.  Also accepts save_model()'s display-key dict (in the
        reference that raises TypeError - SURVEY.md §5)."""
        return cls(**{cls._DISPLAY_KEYS.get(k, k): v for k, v in config.items()})


_PLUGIN_KEYS = ('User Embedding', 'Item Embedding', 'Loss', 'User Initialization', 'Item Initialization')


def _builtin_plugins():
    from . import embedding_graphs, initializer_graphs, loss_graphs
    out = {}
    for mod in (embedding_graphs, initializer_graphs, loss_graphs):
        for name in dir(mod):
            obj = getattr(mod, name)
            if isinstance(obj, type) and obj.__module__ == mod.__name__ and not name.startswith('_'):
                out[name] = obj
    return out


def _encode_plugin(obj, allow_pickle):
    """Built-in plug-in -> {'plugin': class name, 'state': plain data}; anything else only as a pickled object."""
    cls = _builtin_plugins().get(type(obj).__name__)
    if cls is not None and type(obj) is cls:
        state = {}
        for k, v in vars(obj).items():
            if torch.is_tensor(v) or isinstance(v, np.ndarray):
                v = torch.as_tensor(v).detach().cpu()
            elif not isinstance(v, (int, float, bool, str, type(None))):
                raise TypeError(f'{type(obj).__name__}.{k} of type {type(v).__name__} cannot be stored as plain data')
            state[k] = v
        return {'plugin': type(obj).__name__, 'state': state}
    if not allow_pickle:
        raise TypeError(f'{type(obj).__name__} is not a built-in plug-in: pass allow_pickle=True to store it pickled')
    return {'pickled': obj}


def _decode_plugin(entry):
    if 'pickled' in entry:
        return entry['pickled']
    cls = _builtin_plugins()[entry['plugin']]
    obj = cls.__new__(cls)
    for k, v in entry['state'].items():
        setattr(obj, k, v)
    return obj


def _save_to_disk(model, path, include_samples=True, allow_pickle=False):
    config, results = model.save_model()
    config = {k: (_encode_plugin(v, allow_pickle) if k in _PLUGIN_KEYS else v) for k, v in config.items()}
    blob = {'format': 'teamoflow_amd.mf/2', 'config': config,
            'user_embedding': None if model.user_embedding is None else model.user_embedding.detach().float().cpu(),
            'item_embedding': None if model.item_embedding is None else model.item_embedding.detach().float().cpu(),
            'factor_dtype': str(model.factor_dtype).replace('torch.', ''),
            'optimizer': getattr(model, 'optimizer', 'fresh_adam'),
            'user_alpha': float(getattr(model, 'user_alpha', 0.0)), 'item_alpha': float(getattr(model, 'item_alpha', 0.0)),
            'resample_every': int(getattr(model, 'resample_every', 0)), 'sample_seed': int(getattr(model, 'sample_seed', 0)),
            'loss_history': [float(x) for x in (getattr(model, 'loss_history_', []) or [])],
            'random_ind': (torch.as_tensor(model.random_ind).cpu() if include_samples and model.random_ind is not None else None)}
    sampling = (getattr(model, 'negative_sampling', 'uniform'), getattr(model, 'sampling_power', 0.75))
    if sampling != ('uniform', 0.75):   # only then, as below
        blob['negative_sampling'], blob['sampling_power'] = str(sampling[0]), float(sampling[1])
    if getattr(model, 'sampling_correction', 'none') != 'none':   # only then, likewise
        blob['sampling_correction'] = str(model.sampling_correction)
    if model._item_bias_setting():   # only then: a model without the setting writes the file it always wrote
        bias = getattr(model, 'item_bias_', None)
        blob['scalar_item_bias'] = True
        blob['item_bias'] = None if bias is None else bias.detach().float().cpu()
    torch.save(blob, path)


def _load_from_disk(cls, path, device=None, allow_pickle=False):
    blob = torch.load(path, map_location='cpu', weights_only=not allow_pickle)
    if blob.get('format') == 'teamoflow_amd.mf/1':
        raise ValueError(f'{path}: saved by an older version of this package (format /1, pickled plug-ins); load it with that '
                         'version and save it again - the current format /2 stores plain data only')
    if blob.get('format') != 'teamoflow_amd.mf/2':
        raise ValueError(f'{path}: not a teamoflow_amd model file')
    cfg = {k: (_decode_plugin(v) if k in _PLUGIN_KEYS else v) for k, v in blob['config'].items()}
    generate = cfg['Generate Sample']
    cfg['Generate Sample'] = False          # the table comes from the file (or is absent), never redrawn
    model = cls.from_saved(cfg)
    model.generate_sample = generate
    dev = default_device() if device is None else torch.device(device)
    dt = getattr(torch, blob['factor_dtype'])
    model.factor_dtype = dt
    model.optimizer = blob.get('optimizer', 'fresh_adam')
    model.user_alpha, model.item_alpha = float(blob.get('user_alpha', 0.0)), float(blob.get('item_alpha', 0.0))
    model.resample_every, model.sample_seed = int(blob.get('resample_every', 0)), int(blob.get('sample_seed', 0))
    for name in ('user_embedding', 'item_embedding'):
        t = blob[name]
        setattr(model, name, None if t is None else t.to(device=dev, dtype=dt))
    model.user_trainable = [model.user_embedding] if model.user_embedding is not None else None
    model.item_trainable = [model.item_embedding] if model.item_embedding is not None else None
    model.negative_sampling, model.sampling_power = blob.get('negative_sampling', 'uniform'), float(blob.get('sampling_power', 0.75))
    model.sampling_correction = blob.get('sampling_correction', 'none')
    model.scalar_item_bias = bool(blob.get('scalar_item_bias', False))
    bias = blob.get('item_bias')
    model.item_bias_ = None if bias is None else bias.to(device=dev, dtype=torch.float32)
    model.loss_history_ = blob['loss_history']
    if blob['random_ind'] is not None:
        model.random_ind = blob['random_ind'].to(dev)
    return model


def _adam_scalars(lr):
    f = np.float32
    one, b1, b2 = f(1.0), f(0.9), f(0.999)
    return f(f(lr) * np.sqrt(f(one - b2)) / f(one - b1)), f(one - b1), f(one - b2), f(1e-7)
