"""The KernelTimer span names of every epoch - what bench.py and tools/time_*.py read - pinned as exact sets for all ten engine
names, and _engine.run_epoch against the direct epoch_* call: same loss and same tables, bit for bit, from equal starting tables.
TrainState.set_negatives of a KOSWARPLoss state: a fresh state's bits, and nothing allocated by the epoch after it.
_engine.epoch_sides over every pair of side forms: the span names in launch order.
96 users x 64 items, r = 16, S = 8, ~600 interactions of which user 0 has 300 (a row cut into three segments at chunk = 128)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

M, N, R_, S, CHUNK, LR = 96, 64, 16, 8, 128, 0.05
MSE = {'mse_user_pass', 'mse_item_pass'}
KL = {'kl_moments', 'kl_coeffs', 'kl_user_pass', 'kl_item_pass'}
FUSED = {'wmrb_user_pass', 'wmrb_item_pass', 'wmrb_combine'}
SLICED = FUSED | {'wmrb_scores', 'wmrb_hinge', 'wmrb_gradu', 'wmrb_finish'}
LOGISTIC = {'logistic_user_pass', 'logistic_item_pass'}
FSM = {'fsm_lse', 'fsm_user_pass', 'fsm_item_pass', 'fsm_wsum_user', 'fsm_wsum_item', 'fsm_user_step', 'fsm_item_step'}
PAIRS = ('wmrb', 'bpr', 'warp', 'warp_kos', 'softmax')   # the losses over the negative table; all but 'wmrb' on the sliced pass alone
BIAS = {side + name for side in ('user_', 'item_') for name in ('bias_colsum', 'bias_adam', 'adam_bias_rows')}


def pair_spans(*pair_step):
    return (SLICED - {'wmrb_hinge'}) | set(pair_step)


@pytest.fixture(scope='module')
def eng():
    from teamoflow_amd import _engine, _lib
    _lib.get()
    return _engine


@pytest.fixture(scope='module')
def prob():
    g = torch.Generator().manual_seed(11)
    u = torch.cat([torch.zeros(300, dtype=torch.int64), torch.randint(1, M, (300,), generator=g)])
    idx = torch.stack([u, torch.randint(0, N, (600,), generator=g)], 1)
    val = torch.randint(-1, 4, (600,), generator=g).float()          # both KL classes, most of them positives
    R = torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(M)]).to(torch.int32)
    U0, V0 = 0.3 * torch.randn(M, R_, generator=g), 0.3 * torch.randn(N, R_, generator=g)
    return dict(idx=idx.cuda(), val=val.cuda(), R=R.cuda(), U0=U0, V0=V0)


def state(eng, prob, loss, sliced=None, biased=False):
    table = loss in PAIRS
    plan = eng.InteractionPlan(prob['idx'], prob['val'], M, N, chunk=CHUNK, csc=not table)
    assert plan.seg_u.n_long >= 1 and int(plan.rowptr_u[1]) == 300    # user 0's row is cut
    wplan = None
    if table:
        wplan = eng.WmrbPlan(plan, prob['R'], chunk=CHUNK, item_slices=2 if sliced else 1, n_components=R_, sliced=sliced)
    bias = torch.zeros(R_) if biased else None
    return eng.TrainState(prob['U0'], prob['V0'], plan, R_, wplan, kl=loss == 'kl', user_bias=bias, item_bias=bias,
                          full_softmax=loss == 'full_softmax')


def run(eng, st, call):
    """call(st, adam, loss_out, prof) -> (span names, loss, the tables and gradient tables the epoch wrote)."""
    prof, loss = eng.KernelTimer(), torch.zeros(1, dtype=torch.float64, device='cuda')
    call(st, eng.adam_constants(LR), loss, prof)
    torch.cuda.synchronize()
    assert all(b is not None for spans in prof.spans.values() for _, b in spans)     # every bracket was closed
    tables = [t.clone() for t in (st.U, st.V, st.U_nxt, st.V_nxt) if t is not None]
    tables += [t.clone() for side in (st.bias_u, st.bias_v) if side is not None for t in (side.G, side.W, side.b)]
    return set(prof.spans), loss.clone(), tables


def same(a, b):
    return a[0] == b[0] and torch.equal(a[1], b[1]) and len(a[2]) == len(b[2]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


KOS = (3, 4)   # KOSWARPLoss(k=3, n=4)
CASES = [('mse', None, MSE), ('kl', None, KL), ('wmrb', False, FUSED), ('wmrb', True, SLICED), ('logistic', None, LOGISTIC),
         ('logistic_w', None, LOGISTIC), ('bpr', True, pair_spans('bpr_pairs')), ('warp', True, pair_spans('warp_pairs')),
         ('warp_kos', True, pair_spans('kos_weights', 'warp_pairs')), ('softmax', True, pair_spans('softmax_pairs')),
         ('full_softmax', None, FSM)]


@pytest.mark.parametrize('loss,sliced,names', CASES, ids=['mse', 'kl', 'wmrb_fused', 'wmrb_sliced'] + [case[0] for case in CASES[4:]])
def test_span_names_and_run_epoch(eng, prob, monkeypatch, loss, sliced, names):
    """Every engine name: the exact span-name set (pinned from a run of the commit before the loss table existed), and run_epoch
    against the direct epoch call from equal starting tables - the same loss and the same tables, bit for bit."""
    for name in ('TMF_ROW_STATIONARY', 'TMF_SCORES5', 'TMF_SCORES6', 'TMF_ROWS4'):
        monkeypatch.delenv(name, raising=False)
    c = {'wmrb': N / S, 'softmax': N / S, 'warp_kos': KOS}.get(loss, 0.0)   # what travels in c's slot for each loss
    if loss in PAIRS:
        pairs = 'hinge' if loss == 'wmrb' else loss

        def direct(st, adam, out, prof):
            eng.epoch_wmrb(st, adam, c, out, prof=prof, pairs=pairs)
    else:
        direct = {'mse': lambda st, adam, out, prof: eng.epoch_mse(st, adam, out, prof=prof),
                  'kl': lambda st, adam, out, prof: eng.epoch_kl(st, adam, out, prof=prof),
                  'logistic': lambda st, adam, out, prof: eng.epoch_logistic(st, adam, out, False, prof=prof),
                  'logistic_w': lambda st, adam, out, prof: eng.epoch_logistic(st, adam, out, True, prof=prof),
                  'full_softmax': lambda st, adam, out, prof: eng.epoch_full_softmax(st, adam, out, prof=prof)}[loss]
    a = run(eng, state(eng, prob, loss, sliced), direct)
    b = run(eng, state(eng, prob, loss, sliced), lambda st, adam, out, prof: eng.run_epoch(st, adam, out, loss, c, prof=prof))
    assert a[0] == names and b[0] == names
    assert float(a[1]) > 0 and same(a, b)


def test_set_negatives_of_a_kos_state_prepares_the_new_plan(eng, prob):
    """A live KOSWARPLoss state as _fit_sparse builds it, one epoch, set_negatives(second table), one epoch: the bits of a state built
    fresh on that table from the tables the first epoch left (tests/test_gpu_resample.py does this for WARPLoss), and the epoch after
    set_negatives allocates nothing - the rebuilt plan has its sample ranks and its omega buffer before it runs."""
    from teamoflow_amd.mf.loss_graphs import KOSWARPLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions
    dev = torch.device('cuda', torch.cuda.current_device())
    inter = SparseInteractions(prob['idx'], prob['val'], (M, N)).to(dev)
    g = torch.Generator().manual_seed(21)
    T = torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(M)]).to(torch.int32)

    def live(R, U0, V0):
        model = MatrixFactorization(R_, loss_graph=KOSWARPLoss(*KOS), n_users=M, n_items=N, n_samples=S)
        model.random_ind = R
        st, c = model._sparse_state('warp_kos', M, N, inter, U0, V0, dev)
        assert c == KOS and st.wplan.sliced and st.wplan._rank is not None and st.wplan.omega.shape == (st.plan.nnz,)
        return st, model._sparse_step(st, 'warp_kos', c, LR)

    def epoch(st, step, out):
        step(0, out)
        torch.cuda.synchronize()
        allocated = torch.cuda.memory_allocated()   # before the copies below
        return st.U[:, :R_].clone(), st.V[:, :R_].clone(), float(out), allocated
    out = torch.zeros(1, dtype=torch.float64, device='cuda')
    st, step = live(prob['R'], prob['U0'], prob['V0'])
    U1, V1, _, _ = epoch(st, step, out)
    st.set_negatives(T.cuda())
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    got = epoch(st, step, out)
    after = got[3]
    fresh, fresh_step = live(T, U1.cpu(), V1.cpu())
    want = epoch(fresh, fresh_step, out)
    assert got[2] == want[2] and got[2] > 0 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], U1) and torch.equal(st.wplan._rank, fresh.wplan._rank)
    assert st.wplan.omega is not None
    assert after == before, (before, after)


@pytest.mark.parametrize('by_hand', [True, False], ids=['ranked_by_hand', 'ranked_by_the_first_epoch'])
def test_set_negatives_of_a_hand_built_ranked_state(eng, prob, by_hand):
    """A WARP state built without MatrixFactorization, as tools/time_resample_c4.py builds it: wmrb_plan_for(force_sliced=True), then
    sample_rank() by hand - or left to the first epoch -, then TrainState.  set_negatives builds the ranks of the next plan itself: they
    are there straight after the call, the epoch after it allocates nothing, and its bits are those of a state built fresh."""
    g = torch.Generator().manual_seed(22)
    T = torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(M)]).to(torch.int32).cuda()
    plan = eng.InteractionPlan(prob['idx'], prob['val'], M, N, chunk=CHUNK, csc=False)
    adam, out = eng.adam_constants(LR), torch.zeros(1, dtype=torch.float64, device='cuda')

    def build(R, U0, V0, ranked):
        wplan = eng.wmrb_plan_for(plan, R, R_, force_sliced=True)
        if ranked:
            wplan.sample_rank()
        return eng.TrainState(U0, V0, plan, R_, wplan)

    def epoch(st):
        eng.epoch_wmrb(st, adam, 0.0, out, pairs='warp')
        st.swap()
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated()
    st = build(prob['R'], prob['U0'], prob['V0'], by_hand)
    epoch(st)
    U1, V1 = st.U[:, :R_].cpu(), st.V[:, :R_].cpu()
    st.set_negatives(T)
    assert st.wplan._rank is not None and st.wplan.prepared == [('sample_rank', ())]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert epoch(st) == before
    got = float(out)
    fresh = build(T, U1, V1, True)
    epoch(fresh)
    assert float(out) == got and got > 0 and torch.equal(st.U, fresh.U) and torch.equal(st.V, fresh.V)
    assert torch.equal(st.wplan._rank, fresh.wplan._rank)


def test_span_names_of_a_biased_epoch(eng, prob):
    from teamoflow_amd import _lib
    grad = dict(item_epi=_lib.EPI_GRAD, user_epi=_lib.EPI_GRAD)
    a = run(eng, state(eng, prob, 'mse', biased=True), lambda st, adam, out, prof: eng.epoch_sides(st, adam, out, 'mse', prof=prof))
    assert a[0] == MSE | BIAS
    # the passes inside: run_epoch and epoch_mse write the same loss and gradient tables as epoch_sides read them from
    b = run(eng, state(eng, prob, 'mse', biased=True), lambda st, adam, out, prof: eng.epoch_mse(
        st, adam, out, item_out=st.bias_v.G, user_out=st.bias_u.G, prof=prof, **grad))
    d = run(eng, state(eng, prob, 'mse', biased=True), lambda st, adam, out, prof: eng.run_epoch(
        st, adam, out, 'mse', item_out=st.bias_v.G, user_out=st.bias_u.G, prof=prof, **grad))
    assert b[0] == d[0] == MSE and same(b, d)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2][2], b[2][2]) and torch.equal(a[2][5], b[2][5])   # loss, user G, item G


# ------------------------------------------------------------------------------------------------------------------------
# epoch_sides: every ordered pair of side forms
# ------------------------------------------------------------------------------------------------------------------------
N_FEATURES, ALPHA = 24, 0.01
RELU_NAMES = ['relu_dweights', 'relu_dhidden', 'relu_adam_weights', 'relu_bias_colsum', 'relu_bias_adam', 'relu_feat_backward',
              'relu_feat_forward', 'relu_embed']
# form -> (kind of side, penalised, its span names in launch order)
FORMS = {'plain': ('plain', False, []),
         'plain_l2': ('plain', True, ['adam_rows_l2']),
         'biased': ('bias', False, ['bias_colsum', 'bias_adam', 'adam_bias_rows']),
         'biased_l2': ('bias', True, ['bias_colsum', 'bias_adam', 'adam_bias_rows_l2']),
         'featured': ('feat', False, ['feat_backward', 'feat_forward']),
         'featured_l2': ('feat', True, ['feat_backward', 'feat_forward']),
         'relu': ('relu', False, RELU_NAMES)}


def features(rows, seed):
    """[rows, 24] sparse features, two to three entries per row; row 0 has 300 entries, row 2 none.  The side's lists are cut at the
    engine's own chunk of 1024 entries, whatever the chunk of the interaction plan, so that row 0 stays one segment: row 1 has 1100
    entries, the row whose CSR list IS cut into two."""
    from teamoflow_amd.mf.sparse import SparseFeatures
    g = torch.Generator().manual_seed(seed)
    per_row = torch.randint(2, 4, (rows,), generator=g)
    per_row[0], per_row[1], per_row[2] = 300, 1100, 0
    row = torch.repeat_interleave(torch.arange(rows), per_row)
    col = torch.randint(0, N_FEATURES, (row.numel(),), generator=g)
    return SparseFeatures(torch.stack([row, col], 1), torch.randn(row.numel(), generator=g), (rows, N_FEATURES), device='cuda')


@pytest.fixture(scope='module')
def sides_prob(eng, prob):
    """What the 49 states share and leave unchanged: the interaction plan, the feature matrices and the start values of every form."""
    g = torch.Generator().manual_seed(12)
    plan = eng.InteractionPlan(prob['idx'], prob['val'], M, N, chunk=CHUNK, csc=True)
    assert plan.seg_u.n_long >= 1 and int(plan.rowptr_u[1]) == 300    # user 0's row is cut
    out = dict(plan=plan)
    for side, rows, X0 in (('user', M, prob['U0']), ('item', N, prob['V0'])):
        F = features(rows, 13 + rows)
        out[side] = dict(rows=rows, X0=X0, F=F, W0=0.3 * torch.randn(N_FEATURES, R_, generator=g),
                         relu_W0=0.3 * torch.randn(5 * R_, R_, generator=g), relu_Wr0=torch.randn(rows, 5 * R_, generator=g),
                         relu_b0=0.1 * torch.randn(5 * R_, generator=g))
    return out


def sides_state(eng, sp, user_form, item_form):
    """The state of (user form, item form), before set_l2."""
    tables, kw = [], {}
    for side, form in (('user', user_form), ('item', item_form)):
        kind, d = FORMS[form][0], sp[side]
        tables.append({'plain': d['X0'], 'bias': d['X0'], 'feat': d['W0'], 'relu': d['relu_W0']}[kind])
        if kind == 'bias':
            kw[side + '_bias'] = torch.zeros(R_)
        elif kind == 'feat':
            kw[side + '_feat'] = d['F']
        elif kind == 'relu':
            kw[side + '_relu'] = dict(F=None, Wr0=d['relu_Wr0'], b0=d['relu_b0'])   # indicator features
    return eng.TrainState(tables[0], tables[1], sp['plan'], R_, **kw)


def test_epoch_sides_over_every_pair_of_forms(eng, sides_prob):
    """One epoch_sides of each of the 7 x 7 (user form, item form) states: the ordered first occurrences of the span names are the two
    passes, then the user side's step, then the item side's; L2 next to a ReLU side is refused by set_l2.  For (plain penalised,
    featured) - the one pair in which a launch moved when the per-form epoch functions became epoch_sides: the penalised plain side
    used to step after the structured ones - the old sequence by hand leaves the same bits."""
    from teamoflow_amd import _lib
    adam, ran, refused, compared = eng.adam_constants(LR), 0, 0, 0
    for user_form, (user_kind, user_l2, user_names) in FORMS.items():
        for item_form, (item_kind, item_l2, item_names) in FORMS.items():
            what = (user_form, item_form)
            st = sides_state(eng, sides_prob, user_form, item_form)
            alphas = (ALPHA if user_l2 else 0.0, ALPHA if item_l2 else 0.0)
            if 'relu' in (user_kind, item_kind) and any(alphas):
                with pytest.raises(NotImplementedError, match='L2 regularisation next to a ReLU side'):
                    st.set_l2(*alphas)
                refused += 1
                continue
            if any(alphas):
                st.set_l2(*alphas)
            prof, loss = eng.KernelTimer(), torch.zeros(1, dtype=torch.float64, device='cuda')
            eng.epoch_sides(st, adam, loss, 'mse', prof=prof)
            torch.cuda.synchronize()
            assert list(prof.spans) == ['mse_user_pass', 'mse_item_pass'] + ['user_' + x for x in user_names] + \
                ['item_' + x for x in item_names], what
            assert all(b is not None for spans in prof.spans.values() for _, b in spans) and float(loss) > 0, what
            ran += 1
            if what == ('plain_l2', 'featured'):
                old = sides_state(eng, sides_prob, user_form, item_form)
                old.set_l2(*alphas)
                old_loss = torch.zeros(1, dtype=torch.float64, device='cuda')
                eng.run_epoch(old, adam, old_loss, 'mse', 0.0, _lib.EPI_GRAD, old.sides[1].G, None, _lib.EPI_GRAD, old.sides[0].G)
                old.sides[1].step(old.V, old.slab, adam, None, 'item_')
                old.sides[0].step(old.U, old.slab, adam, None, 'user_')
                old.swap()
                torch.cuda.synchronize()
                assert st.U_nxt is None and st.feat_v is st.sides[1] and bool(st.U.isfinite().all())
                assert torch.equal(st.U, old.U) and torch.equal(st.V, old.V) and torch.equal(st.feat_v.W, old.feat_v.W)
                assert torch.equal(loss, old_loss)
                compared += 1
    assert (ran, refused, compared) == (43, 6, 1)   # ReLU beside one of the three penalised forms, on either side: 6 of the 49
