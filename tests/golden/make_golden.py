"""Regenerates the golden fixtures in this directory from the CPU oracle.

    python tests/golden/make_golden.py

The reference itself cannot be imported here (it needs TensorFlow, which is not in the image -
SURVEY.md §8c), so the expected outputs come from ``oracle.dense_ref`` (the dense-faithful,
autograd-differentiated restatement).  The one vector that comes from the reference's own tests
is ``gather_known_answer`` (/root/reference/test/test_utils.py:47-57, also the docstring example
at src/teamoflow/mf/utils.py:68-84) - it is DATA copied from that test, not code.

Inputs use the reference's own generator recipe (``utils.generate_random_interaction`` /
``utils.random_sampler`` restated in ``oracle.datagen``) under a fixed ``np.random.seed``.
Initial weights come from ``oracle.datagen.{normal,uniform}_init`` (TF's RNG stream cannot be
reproduced) and are stored in the fixtures.
"""
import hashlib
import os
import string
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))

from oracle import datagen as G  # noqa: E402
from oracle import dense_ref as D  # noqa: E402
from oracle import sparse_ref as S  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def save(name, **kw):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **kw)
    print(f'{name}: {os.path.getsize(path) / 1024:.1f} KiB')


def gather_known_answer():
    save('gather_known_answer',
         input=np.array([[1, 4, 2], [5, 7, 8], [6, 2, 1]], dtype=np.float32),
         index=np.array([[0, 2, 0], [2, 2, 2], [2, 1, 0]], dtype=np.int64),
         expected=np.array([[1, 2, 1], [8, 8, 8], [1, 2, 6]], dtype=np.float32))


def c1_inputs():
    """BASELINE config 1: 100x50, density .05, r=5, MSE, lr 1e-2 (examples/benchmark_toydata.py:40 call order)."""
    np.random.seed(0)
    idx, val, shape, A = G.generate_random_interaction(100, 50, density=0.05)
    return idx, val, A, G.normal_init(100, 5, 101), G.normal_init(50, 5, 102)


def c1_mse():
    idx, val, A, U0, V0 = c1_inputs()
    epochs = 450
    out = D.fit_dense(U0, V0, idx, val, 'mse', epochs, 1e-2, record_epochs=(1, 2, 25, epochs))
    U, V = out['U'], out['V']
    kw = dict(indices=idx, values=val, A=A, U0=U0, V0=V0, lr=1e-2, loss=out['loss'],
              predictions=D.predict_dense(U, V), top10=D.retrieve_user_recs_dense(U, V, k=10),
              recall10=D.recall_at_k_dense(U, V, A, 10),
              recall10_rows=D.recall_at_k_dense(U, V, A, 10, preserve_rows=True),
              precision10=D.precision_at_k_dense(U, V, A, 10))
    for e, (u, v) in out['snapshots'].items():
        kw[f'U_{e}'], kw[f'V_{e}'] = u, v
    save('c1_mse', **kw)


def wmrb_small_inputs():
    """Shape of the reference's own WMRB smoke test (test/test_loss.py:14-21,50-57):
    50x100, density .05, r=3, S = n_items // 2, lr .1, 25 epochs."""
    np.random.seed(1)
    idx, val, shape, A = G.generate_random_interaction(50, 100, density=0.05)
    R = G.random_sampler(100, 50, 50)
    return idx, val, A, R, G.uniform_init(50, 3, 201), G.uniform_init(100, 3, 202)


def wmrb_small():
    idx, val, A, R, U0, V0 = wmrb_small_inputs()
    out = D.fit_dense(U0, V0, idx, val, 'wmrb', 25, 0.1, random_ind=R, n_items=100, n_samples=50,
                      record_epochs=(1, 2, 25))
    t = S.wmrb_terms(U0, V0, idx, val, R, 100, 50)
    kw = dict(indices=idx, values=val, A=A, R=R, U0=U0, V0=V0, lr=0.1, n_items=100, n_samples=50,
              loss=out['loss'], D_first=t['D'], delta_first=t['delta'], M_first=t['M'],
              recall10=D.recall_at_k_dense(out['U'], out['V'], A, 10),
              top10=D.retrieve_user_recs_dense(out['U'], out['V'], k=10))
    for e, (u, v) in out['snapshots'].items():
        kw[f'U_{e}'], kw[f'V_{e}'] = u, v
    save('wmrb_small', **kw)


def wmrb_mixed_inputs():
    """Mixed-sign interactions (test/test_loss.py:20-21 recipe: min_val=-5): non-positive entries
    must contribute nothing to WMRB but count as hits in recall_at_k."""
    np.random.seed(2)
    idx, val, shape, A = G.generate_random_interaction(40, 60, min_val=-5.0, max_val=5.0, density=0.08)
    R = G.random_sampler(60, 40, 12)
    return idx, val, A, R, G.normal_init(40, 8, 301), G.normal_init(60, 8, 302)


def wmrb_mixed():
    idx, val, A, R, U0, V0 = wmrb_mixed_inputs()
    out = D.fit_dense(U0, V0, idx, val, 'wmrb', 10, 0.05, random_ind=R, n_items=60, n_samples=12,
                      record_epochs=(1, 10))
    outm = D.fit_dense(U0, V0, idx, val, 'mse', 10, 0.05, record_epochs=(1, 10))
    kw = dict(indices=idx, values=val, A=A, R=R, U0=U0, V0=V0, lr=0.05, n_items=60, n_samples=12,
              loss=out['loss'], loss_mse=outm['loss'],
              recall10=D.recall_at_k_dense(out['U'], out['V'], A, 10),
              recall10_rows=D.recall_at_k_dense(out['U'], out['V'], A, 10, preserve_rows=True))
    for e, (u, v) in out['snapshots'].items():
        kw[f'U_{e}'], kw[f'V_{e}'] = u, v
    for e, (u, v) in outm['snapshots'].items():
        kw[f'Um_{e}'], kw[f'Vm_{e}'] = u, v
    save('wmrb_mixed', **kw)


def c2_inputs():
    """BASELINE config 2: 943x1682 (MovieLens-100K shape), r=32, MSE, lr 1e-3, target nnz 100,000
    (density = target / (0.9 m n): the recipe drops the ~10% of entries that round to 0)."""
    m, n = 943, 1682
    np.random.seed(0)
    idx, val, shape, A = G.generate_random_interaction(m, n, density=100000 / (0.9 * m * n))
    return idx, val, A, G.normal_init(m, 32, 401), G.normal_init(n, 32, 402)


def c2_mse():
    idx, val, A, U0, V0 = c2_inputs()
    out = D.fit_dense(U0, V0, idx, val, 'mse', 100, 1e-3, record_epochs=(1, 100))
    U1, V1 = out['snapshots'][1]
    U, V = out['U'], out['V']
    save('c2_mse', nnz=len(val), indices_sha=sha(idx), values_sha=sha(val), U0_sha=sha(U0), V0_sha=sha(V0),
         lr=1e-3, loss=out['loss'], U_1=U1, V_1=V1, U_100_head=U[:64], V_100_head=V[:64],
         recall10_mean=float(D.recall_at_k_dense(U, V, A, 10).mean()),
         top10_head=D.retrieve_user_recs_dense(U, V, k=10)[:64])


def c3r_inputs():
    """Reduced BASELINE config 3 (1/10 linear scale of 6040x3706, r=64, WMRB, S = n // 2, lr .1)."""
    m, n = 604, 371
    np.random.seed(3)
    idx, val, shape, A = G.generate_random_interaction(m, n, density=10000 / (0.9 * m * n))
    R = G.random_sampler(n, m, n // 2)
    return idx, val, A, R, G.uniform_init(m, 64, 501), G.uniform_init(n, 64, 502)


def c3r_wmrb():
    idx, val, A, R, U0, V0 = c3r_inputs()
    m, n = A.shape
    out = D.fit_dense(U0, V0, idx, val, 'wmrb', 20, 0.1, random_ind=R, n_items=n, n_samples=n // 2,
                      record_epochs=(1, 20))
    U1, V1 = out['snapshots'][1]
    save('c3r_wmrb', nnz=len(val), indices_sha=sha(idx), values_sha=sha(val), R_sha=sha(R), U0_sha=sha(U0),
         V0_sha=sha(V0), lr=0.1, loss=out['loss'], U_1=U1, V_1=V1,
         recall10_mean=float(D.recall_at_k_dense(out['U'], out['V'], A, 10).mean()))


def plugin_inputs(seed=7, m=40, n=30, r=6):
    """Small mixed-sign problem with dense NON-identity features for the plug-ins beyond Linear + MSE / WMRB:
    BiasedLinearEmbedding / ReLUEmbedding (embedding_graphs.py:41-87) and KLDivergenceLoss (loss_graphs.py:91-122)."""
    rng = np.random.default_rng(seed)
    A = ((rng.random((m, n)) < 0.3) * rng.integers(-2, 6, (m, n))).astype(np.float32)
    idx, val = np.argwhere(A != 0).astype(np.int64), A[A != 0]
    return dict(A=A, indices=idx, values=val,
                U0=(rng.standard_normal((m, r)) * 0.3).astype(np.float32), V0=(rng.standard_normal((n, r)) * 0.3).astype(np.float32),
                Fu=(np.eye(m) + 0.05 * rng.random((m, m))).astype(np.float32), Fv=(np.eye(n) + 0.05 * rng.random((n, n))).astype(np.float32),
                U0_relu=(rng.standard_normal((5 * r, r)) * 0.3).astype(np.float32),        # ReLUEmbedding: weights are [aux_dim = 5 r, r]
                relu_w0=(rng.standard_normal((m, 5 * r)) * 0.2).astype(np.float32))        # the matrix TF would draw at first use


PLUGIN_CASES = {'plugin_biased': dict(loss='mse', user_embedding='biased', item_embedding='biased'),
                'plugin_relu': dict(loss='mse', user_embedding='relu'),
                'plugin_kl': dict(loss='kl')}
PLUGIN_EPOCHS, PLUGIN_LR = 12, 0.02


def plugin_case(name):
    p = plugin_inputs()
    kw = dict(PLUGIN_CASES[name])
    relu = kw.get('user_embedding') == 'relu'
    out = D.fit_dense_plugins(p['U0_relu'] if relu else p['U0'], p['V0'], p['indices'], p['values'], kw.pop('loss'), PLUGIN_EPOCHS,
                              PLUGIN_LR, p['Fu'], p['Fv'], user_relu_weight0=p['relu_w0'] if relu else None, record_epochs=(1,), **kw)
    fx = dict(p, lr=PLUGIN_LR, epochs=PLUGIN_EPOCHS, loss=out['loss'], user_embedding=out['user_embedding'],
              item_embedding=out['item_embedding'])
    for side, (first, last) in dict(user=(out['snapshots'][1][0], out['user_vars']), item=(out['snapshots'][1][1], out['item_vars'])).items():
        for i, (a, b) in enumerate(zip(first, last)):
            fx[f'{side}_var{i}_1'], fx[f'{side}_var{i}_{PLUGIN_EPOCHS}'] = a, b
    return fx


def plugins():
    for name in PLUGIN_CASES:
        save(name, **plugin_case(name))


# ------------------------------------------------------------------------------------------------------------------------
# fit_routes.json: which trainer MatrixFactorization.fit / fit_als calls, or what it refuses with, over a grid of models
# ------------------------------------------------------------------------------------------------------------------------
ROUTE_LOSSES = ('MSELoss', 'WMRBLoss', 'KLDivergenceLoss', 'LogisticLoss', 'BPRLoss', 'WARPLoss', 'subclass of MSELoss')
ROUTE_SIDES = ('Linear/eye', 'Biased/eye', 'ReLU/eye', 'Linear/SparseFeatures', 'ReLU/SparseFeatures', 'Linear/dense',
               'subclass of Linear/eye')
ROUTE_SETTINGS = (('batch_users', 8), ('shard_items', 2), ('data_parallel', True), ('data_parallel', 'force'),
                  ('factor_dtype', 'bfloat16'), ('optimizer', 'adam'), ('relu_engine', True), ('user_alpha', 0.1),
                  ('resample_every', 3))
ROUTE_ALS_SETTINGS = ROUTE_SETTINGS + (('item_alpha', 0.1),)


def route_setting_combos():
    """No setting, every single one, every unordered pair of two different attributes: 1 + 9 + 35."""
    single = [(s,) for s in ROUTE_SETTINGS]
    pairs = [(a, b) for i, a in enumerate(ROUTE_SETTINGS) for b in ROUTE_SETTINGS[i + 1:] if a[0] != b[0]]
    return [()] + single + pairs


def fit_route_outcomes():
    """What the imported teamoflow_amd does, as {'fit': {'<loss> gpu=<bool>': [outcome per (user side, item side, combo)]},
    'als': {'gpu=<bool>': [outcome per (user side, item side, setting)]}} - an outcome is 'engine' / 'generic' (fit), 'als' (fit_als) or
    'ExceptionType: message'.  The trainers are patched to record their call; no GPU and no libtmf.so is needed."""
    import torch
    from teamoflow_amd import _als
    from teamoflow_amd.mf import embedding_graphs as E, loss_graphs as L
    from teamoflow_amd.mf.initializer_graphs import Initializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseFeatures, SparseInteractions, eye

    class MyMSE(L.MSELoss):
        pass

    class MyLinear(E.LinearEmbedding):
        pass

    class CpuZeros(Initializer):   # the built-in initialisers ask for the current device
        def initialize_weights(self, n_features, n_components):
            return torch.zeros(n_features, n_components)

    m, n, r = 6, 7, 2
    losses = dict(zip(ROUTE_LOSSES, (L.MSELoss, L.WMRBLoss, L.KLDivergenceLoss, L.LogisticLoss, L.BPRLoss, L.WARPLoss, MyMSE)))

    def features(kind, rows):   # built on the CPU, before torch.cuda.is_available is patched
        if kind == 'SparseFeatures':
            own = torch.arange(rows)
            return SparseFeatures(torch.stack([own, (own + 1) % 4], 1), torch.ones(rows), (rows, 4), device='cpu')
        return torch.eye(rows) + 0.5 if kind == 'dense' else eye(rows)
    graphs = {'Linear': E.LinearEmbedding, 'Biased': E.BiasedLinearEmbedding, 'ReLU': E.ReLUEmbedding, 'subclass of Linear': MyLinear}
    sides = [(graphs[s.split('/')[0]], features(s.split('/')[1], m), features(s.split('/')[1], n)) for s in ROUTE_SIDES]
    interactions = SparseInteractions(torch.tensor([[0, 1], [2, 3], [5, 6]]), torch.tensor([1.0, -1.0, 2.0]), (m, n), device='cpu')

    def model(loss, user, item, settings):
        mf = MatrixFactorization(r, user(), item(), loss(), CpuZeros(), CpuZeros(), n_users=m, n_items=n, n_samples=3)
        mf.random_ind, mf.verbose = torch.zeros(m, 3, dtype=torch.int64), False
        for name, value in settings:
            setattr(mf, name, torch.bfloat16 if value == 'bfloat16' else value)
        return mf

    calls = []

    def outcome(call):
        del calls[:]
        try:
            call()
        except Exception as e:   # noqa: BLE001 - the refusal is the record
            return f'{type(e).__name__}: {e}'
        return calls[-1]

    kept = MatrixFactorization._fit_sparse, MatrixFactorization._fit_generic, _als.fit, torch.cuda.is_available
    MatrixFactorization._fit_sparse = lambda self, *a, **k: calls.append('engine') or True
    MatrixFactorization._fit_generic = lambda self, *a, **k: calls.append('generic')
    _als.fit = lambda model, epochs, n_users, n_items, inter, U0, V0, *a: calls.append('als') or (U0, V0)
    out = {'fit': {}, 'als': {}}
    try:
        for gpu in (False, True):
            torch.cuda.is_available = lambda gpu=gpu: gpu
            for name, loss in losses.items():
                out['fit'][f'{name} gpu={gpu}'] = [
                    outcome(lambda: model(loss, ug, ig, combo).fit(1, uf, itf, interactions))
                    for ug, uf, _ in sides for ig, _, itf in sides for combo in route_setting_combos()]
            out['als'][f'gpu={gpu}'] = [
                outcome(lambda: model(L.MSELoss, ug, ig, combo).fit_als(1, uf, itf, interactions))
                for ug, uf, _ in sides for ig, _, itf in sides for combo in [()] + [(s,) for s in ROUTE_ALS_SETTINGS]]
    finally:
        MatrixFactorization._fit_sparse, MatrixFactorization._fit_generic, _als.fit, torch.cuda.is_available = kept
    return out


def fit_routes():
    """Writes fit_routes.json, the record of what the PARENT of the commit that introduced the route table did.  It must be run in
    a worktree of that parent, with this file copied into it (``python tests/golden/make_golden.py fit_routes``), and is never
    regenerated from a later tree: tests/test_fit_routes_cpu.py replays it against the code under test.  Every distinct outcome
    text is stored once; a row is one character: string.ascii_letters[index of its outcome]."""
    import json
    got = fit_route_outcomes()
    texts = sorted({o for part in got.values() for rows in part.values() for o in rows}, key=lambda o: (':' in o, o))
    letter = dict(zip(texts, string.ascii_letters[:len(texts)], strict=True))
    doc = dict(losses=ROUTE_LOSSES, sides=ROUTE_SIDES, settings=[list(s) for s in ROUTE_SETTINGS],
               als_settings=[list(s) for s in ROUTE_ALS_SETTINGS], outcomes=texts,
               **{kind: {key: ''.join(letter[o] for o in rows) for key, rows in part.items()} for kind, part in got.items()})
    path = os.path.join(HERE, 'fit_routes.json')
    with open(path, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    rows = [o for part in got.values() for r in part.values() for o in r]
    print(f'fit_routes: {len(rows)} rows, {len(texts)} outcomes, {os.path.getsize(path) / 1024:.1f} KiB; '
          + ', '.join(f'{rows.count(o)} {o[:40]}' for o in texts[:3]))


# ------------------------------------------------------------------------------------------------------------------------
# kernel_forms.json: which kernel forms _engine chooses for a WMRB fit over a grid of shapes, widths and switches
# ------------------------------------------------------------------------------------------------------------------------
FORM_SHAPES = dict(   # n_users, n_items, n_samples, nnz
    c4=(1_000_000, 100_000, 1024, 100_000_000), c5_shard=(156_250, 1_000_000, 1024, 15_600_000),
    c5_gpu=(1_250_000, 1_000_000, 1024, 124_800_000), c3=(6040, 3706, 1853, 1_000_209), mid=(100_000, 20_000, 256, 5_000_000),
    tiny=(50, 40, 8, 200), past_int32=(3_000_000, 100_000, 1024, 1000))
FORM_WIDTHS = ((8, 'float32'), (64, 'float32'), (100, 'float32'), (128, 'float32'), (200, 'float32'), (256, 'float32'),
               (128, 'bfloat16'), (256, 'bfloat16'))
FORM_SWITCHES = ('TMF_SCORES5', 'TMF_SCORES6', 'TMF_SCORES7', 'TMF_ROW_STATIONARY', 'TMF_ROWS4')
FORM_SETTINGS = ((),) + tuple(((k, v),) for k in FORM_SWITCHES for v in '01') + (
    (('TMF_SCORES5', '1'), ('TMF_SCORES7', '1')), (('TMF_SCORES5', '1'), ('TMF_SCORES6', '1')), (('TMF_SCORES6', '1'), ('TMF_SCORES7', '0')),
    (('TMF_FORCE_SLICED', '1'),), (('TMF_ITEM_SLICES', '7'),))
FORM_SLAB_BUDGET = 64 << 30


def parent_scores_form(eng, m, n, S, nnz, r, dtype, sliced, item_lists):
    """(name, forced) as the parent of the commit that introduced _engine.scores_form launched it: its three predicates over stand-in
    plan objects (a plan 'on the GPU'), the cascade of its TrainState._adopt_wplan and the precedence of its user pass."""
    import torch

    class P:
        pass
    plan, w = P(), P()
    plan.n_items, plan.nnz, plan.n_users, plan.col_u = n, nnz, m, P()
    plan.col_u.is_cuda = True
    w.sliced, w.S, w.R, w.seg_e = sliced, S, torch.zeros(m, S, dtype=torch.int8, device='meta'), (P() if item_lists else None)
    if not sliced:
        return 'scores3', False
    s7 = eng.scores7_wanted(plan, w, r, dtype)
    s6 = not s7 and eng.scores6_wanted(plan, w, r, dtype)
    s5 = w.seg_e is not None and eng.scores5_wanted(plan, w, r, dtype)
    name = 'scores7' if s7 else 'scores6' if s6 else 'scores5' if s5 else 'scores3'
    return name, name != 'scores3' and os.environ.get('TMF_' + name.upper()) == '1'


def kernel_form_outcomes(scores=None):
    """[(outcome text, n_slices)] per case, shape-major, then width, then setting: the scores form and whether its switch forced it
    (``scores``; None: today's _engine.scores_form), row_stationary and rows4 as wmrb_plan_for asks for them, (n_slices, sliced) of
    choose_wmrb_user_pass.  Every case runs with TMF_SLAB_BUDGET = 64 GiB and no other TMF_* variable but its setting's; the
    caller's environment is put back.  Needs libtmf.so's host queries, no GPU."""
    import torch
    from teamoflow_amd import _engine as eng, _lib
    scores = scores or (lambda eng, *a: eng.scores_form(*a[:6], sliced=a[6], on_gpu=True, item_lists=a[7]))
    kept = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith('TMF_') and k != 'TMF_LIB'}
    out = []
    try:
        for m, n, S, nnz in FORM_SHAPES.values():
            for r, dt in FORM_WIDTHS:
                dtype = getattr(torch, dt)
                for setting in FORM_SETTINGS:
                    os.environ.update(dict(setting, TMF_SLAB_BUDGET=str(FORM_SLAB_BUDGET)))
                    ns, sliced = eng.choose_wmrb_user_pass(m, n, _lib.padded_ld(r, dtype), S, nnz, r, elem_size=2 if dt == 'bfloat16' else 4)
                    rs = eng.row_stationary_wanted(m, n, S, nnz, r, dtype, sliced)
                    rows4 = eng.rows4_wanted(r, dtype, n_users=m, n_items=n)
                    name, forced = scores(eng, m, n, S, nnz, r, dtype, sliced, not rows4)
                    flags = [f for f, on in (('forced', forced), ('row_stationary', rs), ('rows4', rows4), ('sliced', sliced)) if on]
                    out.append((' '.join([name] + flags), int(ns)))
                    for k, _ in setting:
                        del os.environ[k]
    finally:
        os.environ.pop('TMF_SLAB_BUDGET', None)
        os.environ.update(kept)
    return out


def kernel_forms():
    """Writes kernel_forms.json, the record of what the PARENT of the commit that introduced _engine.scores_form chose.  Like
    fit_routes: run in a worktree of that parent with this file copied into it (``python tests/golden/make_golden.py kernel_forms``),
    never regenerated from a later tree; tests/test_scores_form_cpu.py replays it.  A row is one character, the index of its outcome
    text, and its slice count."""
    import json
    got = kernel_form_outcomes(parent_scores_form)
    texts = sorted({o for o, _ in got})
    letter = dict(zip(texts, string.ascii_letters[:len(texts)], strict=True))
    doc = dict(shapes={k: list(v) for k, v in FORM_SHAPES.items()}, widths=[list(w) for w in FORM_WIDTHS],
               settings=[[list(kv) for kv in s] for s in FORM_SETTINGS], slab_budget=FORM_SLAB_BUDGET, outcomes=texts,
               rows=''.join(letter[o] for o, _ in got), n_slices=[ns for _, ns in got])
    path = os.path.join(HERE, 'kernel_forms.json')
    with open(path, 'w') as f:
        json.dump(doc, f)
        f.write('\n')
    print(f'kernel_forms: {len(got)} rows, {len(texts)} outcomes, {os.path.getsize(path) / 1024:.1f} KiB; '
          + ', '.join(f"{sum(o.split()[0] == k for o, _ in got)} {k}" for k in ('scores3', 'scores5', 'scores6', 'scores7')))


if __name__ == '__main__':
    if sys.argv[1:] == ['fit_routes']:
        sys.exit(fit_routes())
    if sys.argv[1:] == ['kernel_forms']:
        sys.exit(kernel_forms())
    plugins()
    gather_known_answer()
    c1_mse()
    wmrb_small()
    wmrb_mixed()
    c2_mse()
    c3r_wmrb()
