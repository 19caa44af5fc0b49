"""The training epochs on guarded, poisoned and shared buffers.

Every other test of the epoch kernels runs them on the buffers TrainState allocates: blocks of the caching allocator, rounded up and
laid side by side, fresh or left by the epoch before of the same problem.  A store into row m, into slab slot n_slab or behind
sp[m, S] then lands in slack, and a read of a slot the epoch never wrote finds zeros or the right answer of the last epoch.  Here
``rehome`` moves every buffer an epoch writes, and the tables it reads, of a built TrainState and its WmrbPlan into views of a
tests/arena.py arena - each exactly the size the engine computed, the guard band beginning at the byte behind it - and fills them by
the table BUFFERS below before EVERY epoch.  Each case runs the same two epochs (raw gradients, TMF_EPI_GRAD; then the fresh-Adam
step, TMF_EPI_ADAM) three times - on the state as the engine builds it, re-homed with NaN poison and the NaN band, re-homed with
2^60 and the 2^60 band - and asserts that the bands are intact after every epoch, that every read-only operand kept its bits, that
the loss, the written tables (pad columns included) and the gradient tables agree bit for bit over the three runs, that no poison
is left in an output, that the NaN run meets the fp64 reference of its family at that family's tolerance, and that the case reached
the kernel form its id names.  Then: states that share one scratch (share_scratch's situation), the plan builders of the C ABI on
exact workspaces, and a negative control that shows the guard speaks.

The known remainder: READ overruns of the plan's own index arrays (rowptr, col, the entry lists, the score streams, the slice
offsets) - those arrays stay where the allocator put them.

The problems are small (257 or 513 users, 130 - 260 items, one to three thousand interactions): the whole file takes about six
seconds on an MI355X, no case more than one."""
import collections

import numpy as np
import pytest
import torch

from arena import BIG_BAND, NAN_BAND, Arena, GuardDamaged
from conftest import assert_step, rel_err, step_bounds
from item_bias_ref import biased_reference, margins_decided
from test_bpr_cpu import bpr_closed_form
from test_fullsoftmax_cpu import fullsoftmax_closed_form
from test_fuzz_draws_cpu import BIAS_RTOL, FORM_KEYS
from test_gpu_fuzz_forms import self_pair_floor
from test_kl_cpu import kl_closed_form
from test_kos_cpu import K as KOS_K, N as KOS_N, kos_closed_form, order_decidedness
from test_logistic_cpu import logistic_closed_form
from test_softmax_cpu import softmax_closed_form
from test_warp_cpu import decidedness, warp_closed_form

pytestmark = pytest.mark.gpu

LR = 0.05
CHUNK = 64            # list entries per segment here (the engine's default is 1024): cut rows on both sides at these sizes
F32, BF16 = torch.float32, torch.bfloat16

# ------------------------------------------------------------------------------------------------------------------------
# The initialisation contract of every buffer an epoch writes (INTEGRATION.md prints this table).  'poison': the epoch writes every
# element it later reads, so the buffer may hold anything when the epoch starts - here NaN or 2^60 (0x5a5a5a5a in integer buffers).
# 'zero': a documented caller contract, a kernel relies on it.  'copy': the buffer carries state into the epoch.
# ------------------------------------------------------------------------------------------------------------------------
BUFFERS = {
    'U':          ('copy',   'the user table the epoch reads; never written (full softmax, TMF_EPI_ADAM: stepped in place, see U_nxt)'),
    'V':          ('copy',   'the item table the epoch reads; never written'),
    'U_nxt':      ('poison', 'torch.empty: every row and pad column is stored by the epilogue of the pass that owns the row'),
    'V_nxt':      ('poison', 'torch.empty: likewise, rows of items without an entry included'),
    'slab':       ('poison', 'torch.empty: a slot is stored by its segment before tmf_combine_rows sums the slots of its row'),
    'loss_part':  ('poison', 'torch.zeros, but every pass stores the sum of each segment / user it covers, empty ones included; tmf_sum_f32 '
                             'reads only those'),
    'sp':         ('poison', 'torch.empty: the scores kernel stores the score of every (user, sample)'),
    'pk':         ('poison', 'torch.empty: the scores kernel stores the score of every interaction'),
    'part':       ('poison', 'torch.empty: gradu3 stores a layer per slice; single layer: the launch of the first slice stores, the later ones add'),
    'wbuf':       ('poison', 'torch.zeros, but the pair step stores delta of every interaction (0 for a value <= 0) and D of every sample'),
    'omega':      ('poison', 'torch.empty: tmf_kos_weights stores the weight of every interaction'),
    'rank':       ('copy',   'the sample ranks, written once by the plan with torch and only read by the epochs'),
    'g4_sync':    ('poison', 'torch.zeros, but tmf_wmrb_gradu4 zeroes its counters itself (hipMemsetAsync) in every call'),
    'rows4_sync': ('poison', 'torch.zeros, but tmf_wsum_rows4 / rows5 zero their counters themselves (hipMemsetAsync) in every call'),
    'kl_part':    ('poison', 'torch.zeros, but tmf_kl_moments stores the six moments of every segment'),
    'kl_coef':    ('poison', 'torch.zeros, but tmf_kl_coeffs stores all six coefficients'),
    'fsm_lse':    ('poison', 'torch.zeros, but tmf_fsm_lse_f32 stores the log-partition of every user, those without a positive included'),
    'ib.b':       ('copy',   'the bias the epoch reads; zeros behind n_items'),
    'ib.b_nxt':   ('poison', '[0, n_items) is stored by tmf_item_bias_grad; ZERO behind n_items: a documented contract (the vector is '
                             'also a padded [rows, 4] table), no kernel of the epoch writes there'),
    'ib.ws':      ('poison', 'torch.empty: stage 1 stores the sum of every chunk before stage 2 adds them'),
    'l2.G_user':  ('poison', 'torch.empty: the TMF_EPI_GRAD epilogue stores every row and pad column'),
    'l2.G_item':  ('poison', 'torch.empty: likewise'),
    'grad_U':     ('poison', 'the TMF_EPI_GRAD output table the caller passes in: every row and pad column is stored'),
    'grad_V':     ('poison', 'likewise'),
}


@pytest.fixture(scope='module')
def eng():
    from teamoflow_amd import _engine, _lib
    _lib.get()
    return _engine


# ------------------------------------------------------------------------------------------------------------------------
# problems
# ------------------------------------------------------------------------------------------------------------------------
_PROBLEMS = {}


def make_problem(seed, m, n, r, S, margin=False, heavy=150, per_user=4):
    """Row-major COO pairs without duplicates and the order the engine gets them in (a permutation); values from {-2 .. 5}.  User 0
    is heavy (``heavy`` items), item 1 is popular (every user but two stores it), user ``empty_user`` stores nothing, user
    ``nonpos_user`` only values <= 0, item ``empty_item`` is stored and sampled by nobody.  R [m, S]: ids may repeat inside a row, the
    first sample of a user is one of its positives where it has one, the second (S > 1) the popular item for every third user.
    margin: tables ~ N(0, 1.5 / sqrt(r)) (test_warp_cpu.warp_problem: the margin of 1 neither always nor never holds), else 0.3 N(0, 1)."""
    rng = np.random.default_rng(424200 + seed)
    empty_user, nonpos_user, empty_item, popular = m // 3, m // 2, n // 2, 1
    mask = rng.random((m, n)) < per_user / n
    mask[0, rng.choice(n, min(heavy, n - 1), replace=False)] = True
    mask[:, popular] = True
    mask[empty_user, :] = False
    mask[:, empty_item] = False
    idx = np.argwhere(mask)
    val = rng.choice(np.array([-2, -1, 0, 1, 2, 3, 4, 5], np.float32), idx.shape[0], p=[.06, .06, .08, .16, .16, .16, .16, .16])
    val[idx[:, 0] == nonpos_user] = -np.abs(val[idx[:, 0] == nonpos_user])
    R = rng.integers(0, n, (m, S))
    if S > 1:
        R[::3, 1] = popular
    R[R == empty_item] = (empty_item + 1) % n
    for u in range(m if S else 0):
        mine = idx[(idx[:, 0] == u) & (val > 0), 1]
        if mine.size:
            R[u, 0] = mine[rng.integers(mine.size)]
    scale = np.sqrt(1.5) / r ** 0.25 if margin else 0.3
    U0 = (rng.standard_normal((m, r)) * scale).astype(np.float32)
    V0 = (rng.standard_normal((n, r)) * scale).astype(np.float32)
    b0 = (0.3 * rng.standard_normal(n)).astype(np.float32)
    order = rng.permutation(len(val))
    assert (val > 0).any() and (val <= 0).any() and (order != np.arange(len(val))).any()
    return dict(idx=idx, val=val, U0=U0, V0=V0, b0=b0, R=R.astype(np.int32), S=S, m=m, n=n, r=r, empty_user=empty_user,
                nonpos_user=nonpos_user, empty_item=empty_item, popular=popular, order=order, seed=seed)


def problem_of(case):
    """The problem of a case, made once and left unchanged.  The kinked losses - a first violator, an order statistic - take the first
    seed of a walk whose problem is DECIDED: no fp32 evaluation of a score can choose another first violator (test_warp_cpu.decidedness)
    or order two positives of a user otherwise (test_kos_cpu.order_decidedness; with a bias: item_bias_ref.margins_decided) than fp64."""
    key = (case.loss, case.ib, case.m, case.n, case.r, case.S)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    kinked = case.loss in ('warp', 'warp_kos') or (case.ib and case.loss == 'wmrb')
    # 260 items: the heavy user stores 257 of them - a second pass of the hinge kernel (255 interactions per pass) and its user order
    for seed in range(60):
        # with a bias: the 0.3 N(0, 1) tables of tests/test_gpu_fuzz_bias.py, whose tolerance and gap the bias cases take
        p = make_problem(seed, case.m, case.n, case.r, case.S, margin=kinked and not case.ib, heavy=40 if kinked else 258 if case.n >= 260 else 150,
                         per_user=2 if kinked else 4)
        if not kinked:
            break
        if case.ib:
            scores = p['U0'].astype(np.float64) @ p['V0'].astype(np.float64).T + p['b0'].astype(np.float64)[None, :]
            if margins_decided(scores, p['idx'], p['val'], p['R']):
                break
            continue
        g_min, b = decidedness(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
        if g_min > b and (case.loss != 'warp_kos' or order_decidedness(p['U0'], p['V0'], p['idx'], p['val']) > 2 * b):
            break
    else:
        raise AssertionError(f'no decided problem for {case.id}')
    for a in p.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _PROBLEMS[key] = p
    return p


# ------------------------------------------------------------------------------------------------------------------------
# cases: an explicit covering list.  env: the TMF_* switches that force the form; expect: what the plan and the state must then say
# ------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'id loss m n r S dtype env expect ib l2 part_budget')
SLICED = {'TMF_FORCE_SLICED': '1', 'TMF_SCORES5': '0', 'TMF_SCORES6': '0', 'TMF_SCORES7': '0', 'TMF_ROWS4': '0', 'TMF_ROW_STATIONARY': '0',
          'TMF_USER_CHUNKS': '1'}
S3 = dict(s6=False, s7=False)
S7_ENV = {'TMF_SCORES7': '1', 'TMF_S7_SLICE_BYTES': str(70 * 512), 'TMF_S7_SLOTS': '100'}


def case(id, loss, m, n, r, S, dtype=F32, env=None, expect=None, ib=False, l2=None, part_budget=None, sliced=True):
    base = dict(SLICED) if sliced else {}
    base.update(env or {})
    return Case(id, loss, m, n, r, S, dtype, base, expect or {}, ib, l2, part_budget)


POINTWISE = [
    case('mse-f32-r33', 'mse', 257, 131, 33, 0, sliced=False),
    case('mse-bf16-r256', 'mse', 513, 260, 256, 0, BF16, sliced=False),
    case('mse-f32-r300-wide-rows', 'mse', 257, 130, 300, 0, sliced=False),
    case('mse-f32-r128-user-blocks3', 'mse', 513, 257, 128, 0, env={'TMF_USER_CHUNKS': '3'}, expect=dict(user_chunks=3), sliced=False),
    case('logistic-f32-r100', 'logistic', 513, 200, 100, 0, sliced=False),
    case('logistic_w-bf16-r256', 'logistic_w', 257, 131, 256, 0, BF16, sliced=False),
    case('logistic_w-f32-r300-wide-rows', 'logistic_w', 257, 130, 300, 0, sliced=False),
    case('kl-f32-r33', 'kl', 513, 131, 33, 0, sliced=False),
    case('kl-bf16-r256', 'kl', 257, 260, 256, 0, BF16, sliced=False),
]
WMRB = [
    case('wmrb-fused-f32-r100-S7', 'wmrb', 257, 131, 100, 7, env={'TMF_FORCE_FUSED': '1', 'TMF_ITEM_SLICES': '1', 'TMF_USER_CHUNKS': '1', 'TMF_ROWS4': '0'},
         expect=dict(sliced=False, seg_e_long=True), sliced=False),
    case('wmrb-fused-bf16-r256-S48', 'wmrb', 513, 260, 256, 48, BF16,
         env={'TMF_FORCE_FUSED': '1', 'TMF_ITEM_SLICES': '1', 'TMF_USER_CHUNKS': '2', 'TMF_ROWS4': '0'},
         expect=dict(sliced=False, user_chunks=2), sliced=False),
    case('wmrb-scores3-gradu3-layers-wsum-f32-r33-S1', 'wmrb', 513, 257, 33, 1, env={'TMF_ITEM_SLICES': '3'},
         expect=dict(S3, rs=False, part_layers=3, rows4=False, seg_e_long=True)),
    case('wmrb-scores3-gradu3-single-layer-wsum-bf16-r256-S48', 'wmrb', 257, 131, 256, 48, BF16, env={'TMF_ITEM_SLICES': '2', 'TMF_USER_CHUNKS': '2'},
         expect=dict(S3, rs=False, part_layers=1, rows4=False, user_chunks=2), part_budget=1024),
    case('wmrb-scores6-gradu4-rows4-f32-r128-S7', 'wmrb', 513, 260, 128, 7,
         env={'TMF_SCORES6': '1', 'TMF_S6_SLICE_BYTES': '40000', 'TMF_ROW_STATIONARY': '1', 'TMF_ROWS4': '1', 'TMF_ROWS5': '0', 'TMF_ITEM_SLICES': '3',
              'TMF_USER_CHUNKS': '2'},
         expect=dict(s6=True, s7=False, rs=True, rows4=True, vrows=False, hinge_order=True)),
    case('wmrb-scores6-gradu4-rows5-cut-bf16-r256-S48', 'wmrb', 257, 260, 256, 48, BF16,
         env={'TMF_SCORES6': '1', 'TMF_ROW_STATIONARY': '1', 'TMF_ROWS4': '1', 'TMF_ROWS5_TARGET': '40', 'TMF_ITEM_SLICES': '2', 'TMF_USER_CHUNKS': '3'},
         expect=dict(s6=True, s7=False, rs=True, rows4=True, vrows=True, vrows_long=True)),
    case('wmrb-scores7-gradu3-single-layer-rows5-cut-f32-r100-S48', 'wmrb', 513, 200, 100, 48,
         env=dict(S7_ENV, TMF_S7_FILL='0', TMF_ROWS4='1', TMF_ROWS5_TARGET='100', TMF_ITEM_SLICES='4', TMF_USER_CHUNKS='2'),
         expect=dict(s6=False, s7=True, fill=False, rs=False, part_layers=1, rows4=True, vrows=True, vrows_long=True), part_budget=1024),
    case('wmrb-scores7fill-gradu4-wsum-f32-r128-S7', 'wmrb', 513, 131, 128, 7,
         env=dict(S7_ENV, TMF_S7_FILL='1', TMF_ROW_STATIONARY='1', TMF_ITEM_SLICES='2', TMF_USER_CHUNKS='3'),
         expect=dict(s6=False, s7=True, fill=True, rs=True, rows4=False, user_chunks=3)),
    case('wmrb-scores3-gradu4-rows4-bf16-r256-S7', 'wmrb', 513, 131, 256, 7, BF16,
         env={'TMF_ROW_STATIONARY': '1', 'TMF_ROWS4': '1', 'TMF_ROWS5': '0', 'TMF_ITEM_SLICES': '5'},
         expect=dict(S3, rs=True, rows4=True, vrows=False)),
]
PAIRS = [
    case('bpr-scores3-f32-r33-S7', 'bpr', 257, 131, 33, 7, env={'TMF_ITEM_SLICES': '2'}, expect=dict(S3, seg_e_long=True)),
    case('bpr-scores7fill-f32-r100-S48', 'bpr', 513, 260, 100, 48, env=dict(S7_ENV, TMF_S7_FILL='1', TMF_ITEM_SLICES='3'),
         expect=dict(s7=True, fill=True)),
    case('warp-scores3-f32-r128-S48', 'warp', 257, 200, 128, 48, env={'TMF_ITEM_SLICES': '3'}, expect=dict(S3)),
    case('warp-scores7-f32-r100-S7', 'warp', 513, 131, 100, 7, env=dict(S7_ENV, TMF_S7_FILL='0', TMF_ITEM_SLICES='2'), expect=dict(s7=True, fill=False)),
    case('warp_kos-scores3-f32-r33-S48', 'warp_kos', 257, 260, 33, 48, env={'TMF_ITEM_SLICES': '2'}, expect=dict(S3)),
    case('warp_kos-scores7fill-f32-r100-S7', 'warp_kos', 257, 131, 100, 7, env=dict(S7_ENV, TMF_S7_FILL='1', TMF_ITEM_SLICES='1'),
         expect=dict(s7=True, fill=True)),
    case('softmax-scores3-f32-r100-S1', 'softmax', 513, 131, 100, 1, env={'TMF_ITEM_SLICES': '4', 'TMF_USER_CHUNKS': '2'}, expect=dict(S3, user_chunks=2)),
    case('softmax-scores7-f32-r128-S48', 'softmax', 257, 257, 128, 48, env=dict(S7_ENV, TMF_S7_FILL='0', TMF_ITEM_SLICES='2'),
         expect=dict(s7=True, fill=False)),
    case('bpr-scores3-bf16-r256-S7', 'bpr', 257, 131, 256, 7, BF16, env={'TMF_ITEM_SLICES': '2'}, expect=dict(S3)),
]
OTHER = [
    case('item_bias-wmrb-scores3-f32-r33-S7', 'wmrb', 257, 131, 33, 7, env={'TMF_ITEM_SLICES': '2'}, expect=dict(S3), ib=True),
    case('item_bias-warp-scores7fill-f32-r100-S7', 'warp', 257, 200, 100, 7, env=dict(S7_ENV, TMF_S7_FILL='1', TMF_ITEM_SLICES='2', TMF_USER_CHUNKS='2'),
         expect=dict(s7=True, fill=True, user_chunks=2), ib=True),
    case('item_bias-softmax-scores6-f32-r128-S48', 'softmax', 513, 257, 128, 48, env={'TMF_SCORES6': '1', 'TMF_ITEM_SLICES': '3'},
         expect=dict(s6=True, s7=False), ib=True),
    case('full_softmax-f32-r33-300x257', 'full_softmax', 300, 257, 33, 0, sliced=False),
    case('full_softmax-f32-r128-300x257', 'full_softmax', 300, 257, 128, 0, sliced=False),
    case('l2-both-sides-mse-f32-r100', 'mse', 257, 131, 100, 0, l2=(0.3, 0.7), sliced=False),
    case('l2-both-sides-wmrb-scores3-bf16-r256-S7', 'wmrb', 257, 131, 256, 7, BF16, env={'TMF_ITEM_SLICES': '2'}, expect=dict(S3), l2=(0.3, 0.7)),
]
CASES = POINTWISE + WMRB + PAIRS + OTHER


# ------------------------------------------------------------------------------------------------------------------------
# building and re-homing a state
# ------------------------------------------------------------------------------------------------------------------------
def set_forms(monkeypatch, eng, case):
    """Every form variable cleared, the case's own set.  TMF_PART_BUDGET is read once, when the engine is imported: a case that wants
    the single-layer form of gradu3 sets the variable AND the constant it became."""
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if case.part_budget is not None:
        monkeypatch.setenv('TMF_PART_BUDGET', str(case.part_budget))
        monkeypatch.setattr(eng, 'PART_BUDGET', int(case.part_budget))


def wmrb_plan(eng, plan, R, r, dtype, force_sliced, chunk=CHUNK):
    """_engine.wmrb_plan_for - every choice made by the engine's own choosers from the shape and the switches - with the entry lists cut
    every ``chunk`` entries in place of the default 1024, so that cut list rows occur at these sizes."""
    from teamoflow_amd import _lib
    m, n, S = plan.n_users, plan.n_items, int(R.shape[1])
    ns, sliced = eng.choose_wmrb_user_pass(m, n, _lib.padded_ld(r, dtype), S, plan.n_pos, r, elem_size=2 if dtype is BF16 else 4)
    sliced = sliced or bool(force_sliced)
    rs = eng.row_stationary_wanted(m, n, S, plan.nnz, r, dtype, sliced)
    rows4 = eng.rows4_wanted(r, dtype, plan, R)
    C = eng.rows5_user_chunks(m, r, dtype) if rows4 else eng.default_user_chunks(m, _lib.padded_ld(r), n_items=n)
    wplan = eng.WmrbPlan(plan, R, chunk=chunk, user_chunks=C, item_slices=ns, n_components=r, sliced=sliced, rows4=rows4)
    wplan.row_stationary = rs
    return wplan


def build_state(eng, monkeypatch, case, p, scratch=None):
    set_forms(monkeypatch, eng, case)
    rec, dev, o = eng.LOSSES[case.loss], 'cuda', p['order']
    plan = eng.InteractionPlan(torch.tensor(p['idx'][o], device=dev), torch.tensor(p['val'][o], device=dev), case.m, case.n, chunk=CHUNK,
                               **rec.plan_form())
    wplan = None
    if rec.table:
        wplan = wmrb_plan(eng, plan, eng.checked_negatives(np.array(p['R']), case.m, case.n, dev), case.r, case.dtype, rec.sliced_only or case.ib)
        rec.prepare(wplan, plan)
    kw = dict(kl=True) if rec.flag == 'kl' else dict(full_softmax=True) if rec.flag == 'full_softmax' else {}
    if case.ib:
        kw['item_scalar_bias'] = np.array(p['b0'])
    st = eng.TrainState(torch.tensor(p['U0'], device=dev), torch.tensor(p['V0'], device=dev), plan, case.r, wplan, dtype=case.dtype,
                        scratch=scratch, **kw)
    if case.l2:
        st.set_l2(*case.l2)
    return st


def forms_of(st):
    """What the plan and the state say about the forms the epoch will take."""
    plan, w = st.plan, st.wplan
    f = dict(user_chunks=plan.user_chunks if w is None else w.user_chunks, seg_u_long=plan.seg_u.n_long >= 1)
    if plan.seg_i is not None:
        f['seg_i_long'] = plan.seg_i.n_long >= 1
    if w is not None:
        f.update(sliced=w.sliced, rows4=w.rows4, vrows=w.vrows is not None, vrows_long=w.vrows is not None and w.vrows.n_long >= 1,
                 seg_e_long=w.seg_e is not None and w.seg_e.n_long >= 1, slices=w.n_slices, hinge_order=w.hinge_order is not None)
        if w.sliced:
            f.update(s6=w.s6 is not None, s7=w.s7 is not None, s5=w.s5 is not None, fill=w.s7 is not None and w.s7.sub_wave is not None,
                     rs=bool(st.row_stationary), part_layers=st.part_layers)
    return f


def rehome(st, arena):
    """Moves every buffer an epoch of ``st`` writes, and the tables it reads, into views of ``arena`` of exactly the size the engine
    computed, by assignment, each filled by its row of BUFFERS with the arena's poison; -> {BUFFERS name: view}.  Nothing caches a
    pointer to one of them: SegmentTable.cstruct and WmrbPlan.lists hold index arrays only, and the launchers read the attributes
    assigned here when they launch."""
    from teamoflow_amd import _lib
    L, got = _lib.load_library(), {}

    def take(name, like=None, shape=None, dtype=None, fill=None):
        shape = tuple(like.shape) if shape is None else shape
        dtype = like.dtype if dtype is None else dtype
        kind = BUFFERS[name][0] if fill is None else fill
        got[name] = arena.take(name, shape, dtype, like if kind == 'copy' else kind)
        return got[name]

    st.U, st.V = take('U', st.U), take('V', st.V)
    if st.U_nxt is not None:
        st.U_nxt = take('U_nxt', st.U_nxt)
    if st.V_nxt is not None:
        st.V_nxt = take('V_nxt', st.V_nxt)
    bufs = {k: take(k, shape=(v,), dtype=F32) for k, v in st._need.items()}   # the scratch, through the engine's own binder
    st._bind(bufs)
    st._bufs = bufs
    w = st.wplan
    if w is not None:
        nnz, (m, S) = st.plan.nnz, w.R.shape
        w.wbuf = take('wbuf', w.wbuf)
        w.delta, w.D = w.wbuf[:nnz], w.wbuf[nnz:].view(m, S)
        if getattr(w, 'omega', None) is not None:
            w.omega = take('omega', w.omega)
        if getattr(w, '_rank', None) is not None:
            w._rank = take('rank', w._rank)
        if w.sliced and st.row_stationary:
            nb = L.tmf_wmrb_gradu4_workspace_bytes(m, w.n_slices, st.users_per_launch)
            assert nb >= 4 and nb % 4 == 0
            st.g4_sync = take('g4_sync', shape=(nb // 4,), dtype=torch.int32)
        if w.rows4:
            n_work = w.vrows.n_vrows if w.vrows is not None else st.plan.n_items
            nb = L.tmf_wsum_rows4_workspace_bytes(n_work, w.user_chunks, st.rows4_per_launch)
            assert nb >= 4 and nb % 4 == 0
            st.rows4_sync = take('rows4_sync', shape=(nb // 4,), dtype=torch.int32)
    for name in ('kl_part', 'kl_coef', 'fsm_lse'):
        if getattr(st, name, None) is not None:
            setattr(st, name, take(name, getattr(st, name)))
    if st.ib is not None:
        ib = st.ib
        ib.b, ib.b_nxt = take('ib.b', ib.b), take('ib.b_nxt', ib.b_nxt)
        nb = L.tmf_item_bias_grad_workspace_bytes(ib.n, w.user_chunks, ib.n_extra)
        assert nb >= 8 and nb % 8 == 0
        ib.ws = take('ib.ws', shape=(nb // 8,), dtype=torch.float64)
    for side, name in zip(st.sides, ('l2.G_user', 'l2.G_item')):
        if side is not None:
            side.G = take(name, side.G)
    st._arena_views = got
    return got


def fill_by_contract(st, arena):
    """Before an epoch: every 'poison' buffer poisoned again, every 'zero' contract restored; 'copy' buffers stay."""
    for name, view in st._arena_views.items():
        if BUFFERS[name][0] == 'poison':
            view.fill_(arena.poison_of(view.dtype))
    if st.ib is not None:
        st.ib.b_nxt[st.ib.n:].zero_()


def epoch_operands(st, outs):
    """Every buffer the next epoch of ``st`` hands to a kernel for writing, and the tables it reads."""
    w, t = st.wplan, [st.U, st.V, st.U_nxt, st.V_nxt, st.slab, st.loss_part, *outs]
    if w is not None:
        t += [w.wbuf, w.delta, w.D, getattr(w, 'omega', None), getattr(w, '_rank', None)]
        if w.sliced:
            t += [st.sp, st.pk, st.part, st.g4_sync if st.row_stationary else None]
        t += [st.rows4_sync if w.rows4 else None]
    t += [getattr(st, n, None) for n in ('kl_part', 'kl_coef', 'fsm_lse')]
    if st.ib is not None:
        t += [st.ib.b, st.ib.b_nxt, st.ib.ws]
    t += [side.G for side in st.sides if side is not None]
    return [x for x in t if x is not None and x.numel()]


def read_only(st):
    """name -> tensor of every operand an epoch only reads: the index arrays of the plans (the tables are added by the caller)."""
    p, w = st.plan, st.wplan
    ro = dict(col_u=p.col_u, val_u=p.val_u, rowptr_u=p.rowptr_u)
    if p.seg_i is not None:
        ro.update(row_i=p.row_i, val_i=p.val_i, rowptr_i=p.rowptr_i)
    if w is not None:
        ro.update(R=w.R, ent_row=w.ent_row, ent_w=w.ent_w, rowptr_e=w.rowptr_e)
        if getattr(w, '_rank', None) is not None:
            ro['rank'] = w._rank
    if st.ib is not None:
        ro['b'] = st.ib.b
    return ro


def bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def loss_param(case):
    if case.loss == 'wmrb':
        return case.n / case.S
    if case.loss == 'warp_kos':
        return (KOS_K, KOS_N)
    return 1.0 if case.loss == 'softmax' else 0.0


def run(eng, monkeypatch, case, p, band=None):
    """The two epochs of a case on a fresh state: band None = the buffers the engine allocates, else re-homed into an arena with that
    band and its poison.  -> (outputs: name -> tensor or float, forms, the state)."""
    from teamoflow_amd import _lib
    st = build_state(eng, monkeypatch, case, p)
    forms = forms_of(st)
    dev, adam, c = 'cuda', eng.adam_constants(LR), loss_param(case)
    m, n, ld = case.m, case.n, st.ld
    arena = None
    if band is not None:
        arena = Arena(dev, band)
        rehome(st, arena)
    out = {}
    ro = {k: (v, bits(v).clone()) for k, v in read_only(st).items()}
    tables = {'U': (st.U, bits(st.U).clone()), 'V': (st.V, bits(st.V).clone())}

    def guarded_epoch(tag, call, outs, tables_stay=True):
        if arena is not None:
            fill_by_contract(st, arena)
            for t in epoch_operands(st, outs):
                assert arena.holds(t), (case.id, tag, 'an operand of the epoch lies outside the arena', tuple(t.shape), t.dtype)
        call()
        torch.cuda.synchronize()
        if arena is not None:
            arena.check()
        for k, (t, before) in list(ro.items()) + (list(tables.items()) if tables_stay else []):
            assert torch.equal(bits(t), before), (case.id, tag, f'the epoch changed its read-only operand {k}')

    def grad_tables():
        if arena is None:
            return torch.full((m, ld), 7.0, device=dev), torch.full((n, ld), 7.0, device=dev)
        gU, gV = arena.take('grad_U', (m, ld), F32), arena.take('grad_V', (n, ld), F32)
        st._arena_views.update(grad_U=gU, grad_V=gV)
        return gU, gV

    loss = torch.zeros(2, dtype=torch.float64, device=dev)
    if case.l2:
        # a penalised plain side has one epoch: the raw gradients into the sides' tables, then the regularised step in place
        guarded_epoch('l2', lambda: eng.epoch_sides(st, adam, loss[:1], case.loss, c), [], tables_stay=False)
        out.update(loss1=float(loss[0]), gU=st.sides[0].G.clone(), gV=st.sides[1].G.clone(), U1=st.U.clone(), V1=st.V.clone())
    else:
        gU, gV = grad_tables()
        if st.ib is not None:
            st.ib.epi = _lib.EPI_GRAD
        guarded_epoch('grad', lambda: eng.run_epoch(st, adam, loss[:1], case.loss, c, _lib.EPI_GRAD, gV, None, _lib.EPI_GRAD, gU), [gU, gV])
        out.update(loss1=float(loss[0]), gU=gU.clone(), gV=gV.clone())
        if st.ib is not None:
            out['gb'] = st.ib.b_nxt.clone()
            st.ib.epi = _lib.EPI_ADAM
        if st.wplan is not None:
            out.update(delta=st.wplan.delta.clone(), D=st.wplan.D.clone())
        # the full softmax steps the table it read in place and hands the names over: the stepped tables are U_nxt / V_nxt afterwards
        guarded_epoch('adam', lambda: eng.run_epoch(st, adam, loss[1:], case.loss, c), [], tables_stay=case.loss != 'full_softmax')
        out.update(loss2=float(loss[1]), U1=st.U_nxt.clone(), V1=st.V_nxt.clone())
        if st.ib is not None:
            out['b1'] = st.ib.b_nxt.clone()
    out['U_stored'], out['V_stored'] = tables['U'][1].view(st.dtype).view(m, ld).clone(), tables['V'][1].view(st.dtype).view(n, ld).clone()
    return out, forms, st, arena


def assert_no_poison(case, out, what):
    for k, v in out.items():
        if isinstance(v, torch.Tensor):
            v = v.double()
            assert bool(torch.isfinite(v).all()) and float(v.abs().max()) < 2.0 ** 40, (case.id, what, f'poison left in {k}')
        else:
            assert np.isfinite(v) and abs(v) < 2.0 ** 40, (case.id, what, k, v)


def assert_pads_zero(case, out, r):
    for k in ('gU', 'gV', 'U1', 'V1'):
        assert not bool(out[k][:, r:].any()), (case.id, f'pad columns of {k}')
    for k in ('gb', 'b1'):      # the scalar item bias: zeros behind n_items
        assert k not in out or not bool(out[k][case.n:].any()), (case.id, f'{k} behind n_items')


# ------------------------------------------------------------------------------------------------------------------------
# the references: the fp64 closed form each family's own file uses, at that file's tolerance
# ------------------------------------------------------------------------------------------------------------------------
def reference(eng, case, p, U64, V64):
    """-> dict(loss = the sum the epoch leaves in loss_out, gU, gV[, gb], rtol[, slack_U, slack_V]) on the tables as stored."""
    from oracle import sparse_ref as SR
    idx, val, R, n, S = p['idx'], p['val'], p['R'], case.n, case.S
    v64 = val.astype(np.float64)
    if case.ib:
        from teamoflow_amd.mf import loss_graphs
        kind = dict(wmrb='WMRBLoss', warp='WARPLoss', softmax='SampledSoftmaxLoss')[case.loss]
        ref = biased_reference(getattr(loss_graphs, kind)(), U64, V64, p['b0'], np.array(idx), np.array(val), np.array(R), n, S)
        return dict(loss=ref['loss_sum'], gU=ref['gU'], gV=ref['gV'], gb=ref['gb'], rtol=BIAS_RTOL[case.loss])
    if case.loss == 'mse':
        _, _, mean, t = SR.mse_epoch(U64, V64, idx, v64, LR)
        return dict(loss=mean * len(val), gU=t['gU'], gV=t['gV'], rtol=1e-5)
    if case.loss == 'wmrb':
        _, _, mean, t = SR.wmrb_epoch(U64, V64, idx, v64, R.astype(np.int64), n, S, LR)
        sl = SR.wmrb_slack(U64, V64, idx, v64, R.astype(np.int64), n, S)
        fU, fV = self_pair_floor(n / S, U64, V64)
        # tests/test_gpu_fuzz_forms.py: the weight c / (1 + c M) moves by c times the fp32 rounding of a score
        return dict(loss=mean * int((val > 0).sum()), gU=t['gU'], gV=t['gV'], rtol=1e-5 + 5e-7 * (n / S), slack_U=sl['gU'] + fU, slack_V=sl['gV'] + fV)
    if case.loss in ('logistic', 'logistic_w'):
        loss, gU, gV, _ = logistic_closed_form(U64, V64, idx, val, case.loss == 'logistic_w')
    elif case.loss == 'kl':
        loss, gU, gV, _ = kl_closed_form(U64, V64, idx, val)
    elif case.loss == 'full_softmax':
        loss, gU, gV = fullsoftmax_closed_form(U64, V64, idx, val)
    elif case.loss == 'bpr':
        loss, _, _, gU, gV = bpr_closed_form(U64, V64, idx, val, R)
    elif case.loss == 'warp':
        loss, _, _, gU, gV = warp_closed_form(U64, V64, idx, val, R)
    elif case.loss == 'warp_kos':
        loss, _, _, gU, gV = kos_closed_form(U64, V64, idx, val, R)
    else:
        loss, _, _, gU, gV = softmax_closed_form(U64, V64, idx, val, R, 1.0)
    return dict(loss=loss, gU=gU, gV=gV, rtol=1e-5)


def assert_meets_reference(eng, case, p, out):
    r = case.r
    U64, V64 = out['U_stored'][:, :r].double().cpu().numpy(), out['V_stored'][:, :r].double().cpu().numpy()
    ref = reference(eng, case, p, U64, V64)
    rtol = ref['rtol']
    l2 = [np.float32(2.0 * a).astype(np.float64) for a in (case.l2 or (0.0, 0.0))]
    figures = dict(loss=rel_err(out['loss1'], ref['loss']))
    for name, W64, l2k in (('gU', U64, l2[0]), ('gV', V64, l2[1])):
        g, slack = out[name][:, :r].double().cpu().numpy(), ref.get('slack_' + name[1])
        d = np.abs(g - ref[name]) - (1.0001 * slack if slack is not None else 0.0)
        figures[name] = max(float(d.max()), 0.0) / max(np.abs(ref[name]).max(), 1e-30)
        g_step = ref[name] + l2k * W64                                       # what the table steps from: g + l2 w (set_l2)
        W1 = out[name.replace('g', '') + '1'][:, :r].double().cpu().numpy()
        lo, hi = step_bounds(W64, g_step, LR, rtol, slack)
        if case.dtype is BF16:   # the stepped value lies in [lo, hi]; rounding to nearest bf16 (8 significant bits: unit roundoff 2^-8) is monotone
            lo, hi = lo - 2.0 ** -8 * np.abs(lo), hi + 2.0 ** -8 * np.abs(hi)
        bad = (W1 < lo) | (W1 > hi)
        assert not bad.any(), (case.id, f'{name[1]}: {int(bad.sum())} of {bad.size} elements outside the step interval, first at {tuple(np.argwhere(bad)[0])}')
    if 'gb' in ref:
        figures['gb'] = rel_err(out['gb'][:case.n].double().cpu().numpy(), ref['gb'])
        assert_step(out['b1'][:case.n].cpu().numpy(), p['b0'], ref['gb'], LR, rtol=rtol, what=f'{case.id} b')
    print(f'[train buffers] {case.id}: ' + ' '.join(f'{k} {v:.3g}' for k, v in figures.items()) + f' (rtol {rtol:.3g})')
    assert max(figures.values()) < rtol, (case.id, figures, rtol)
    if 'loss2' in out:
        assert out['loss2'] == out['loss1'], case.id                          # the two epochs read the same tables


def assert_same_bits(case, a, b, what):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(bits(a[k]), bits(b[k])), (case.id, f'{k} differs between {what}')
        else:
            assert a[k] == b[k], (case.id, f'{k} differs between {what}', a[k], b[k])


def assert_forms(case, forms):
    assert forms.get('s5') in (None, False), (case.id, forms)
    for k, v in case.expect.items():
        assert forms.get(k) == v, (case.id, f'the case did not reach the form it names: {k}={forms.get(k)!r}, wanted {v!r}', forms)
    rec_table = 'sliced' in forms
    if not rec_table:      # the list losses: cut rows on both sides
        assert forms['seg_u_long'] and forms['seg_i_long'], (case.id, forms)
    elif not forms['rows4']:
        assert forms['seg_e_long'], (case.id, forms)                          # a cut list row: a slab slot and tmf_combine_rows


@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_epochs_on_guarded_poisoned_buffers(eng, monkeypatch, case):
    p = problem_of(case)
    plain, forms, _, _ = run(eng, monkeypatch, case, p)
    assert_forms(case, forms)
    nan, forms_nan, st, arena = run(eng, monkeypatch, case, p, NAN_BAND)
    assert forms_nan == forms
    assert_no_poison(case, nan, 'NaN poison')
    assert_pads_zero(case, nan, case.r)
    assert_meets_reference(eng, case, p, nan)            # on a re-homed run: bit-equality with a wrong plain run is no pass
    assert_same_bits(case, plain, nan, 'the engine\'s own buffers and the arena with NaN poison')
    # what the families' own files ask of rows without a gradient: they keep their bits (a penalised row decays instead)
    if not case.l2 and case.loss != 'kl':
        for user in (p['empty_user'], p['nonpos_user'])[:1 if case.loss in ('mse', 'logistic', 'logistic_w') else 2]:
            assert not bool(nan['gU'][user].any()) and torch.equal(bits(nan['U1'][user]), bits(nan['U_stored'][user])), (case.id, user)
        if case.loss != 'full_softmax':   # there every item has a gradient from every user with a positive
            assert not bool(nan['gV'][p['empty_item']].any()) and torch.equal(bits(nan['V1'][p['empty_item']]), bits(nan['V_stored'][p['empty_item']])), case.id
    del st, arena
    big, forms_big, _, _ = run(eng, monkeypatch, case, p, BIG_BAND)
    assert forms_big == forms
    assert_no_poison(case, big, '2^60 poison')
    assert_same_bits(case, nan, big, 'NaN poison and 2^60 poison')


# ------------------------------------------------------------------------------------------------------------------------
# states that share one scratch
# ------------------------------------------------------------------------------------------------------------------------
SHARED = (case('shared-large', 'wmrb', 513, 260, 100, 7, env={'TMF_ITEM_SLICES': '3'}, expect=dict(S3)),
          case('shared-small', 'wmrb', 257, 131, 100, 7, env={'TMF_ITEM_SLICES': '3'}, expect=dict(S3)))


def one_epoch(eng, st, case):
    loss = torch.zeros(1, dtype=torch.float64, device='cuda')
    eng.run_epoch(st, eng.adam_constants(LR), loss, case.loss, loss_param(case))
    torch.cuda.synchronize()
    return dict(loss=float(loss), U1=st.U_nxt.clone(), V1=st.V_nxt.clone(), delta=st.wplan.delta.clone(), D=st.wplan.D.clone())


@pytest.mark.parametrize('band', [NAN_BAND, BIG_BAND], ids=['nan', '2^60'])
@pytest.mark.parametrize('first', ['large-first', 'small-first'])
def test_states_that_share_one_scratch(eng, monkeypatch, first, band):
    """share_scratch's situation: two states of different m and nnz bound to ONE set of scratch buffers of the larger size.  Whatever
    the other state's epoch left there - and the poison it never overwrote - a state's epoch gives the bits it gives on scratch of its
    own."""
    ps = [problem_of(c) for c in SHARED]
    own = [one_epoch(eng, build_state(eng, monkeypatch, c, p), c) for c, p in zip(SHARED, ps)]
    scratch = {}
    states = [build_state(eng, monkeypatch, c, p, scratch=scratch) for c, p in zip(SHARED, ps)]
    assert scratch['states'] == states and states[0].plan.nnz != states[1].plan.nnz and states[0].plan.n_users != states[1].plan.n_users
    sizes = {}
    for st in states:
        for k, v in st._need.items():
            sizes[k] = max(sizes.get(k, 0), v)
    assert all(sizes[k] > states[1]._need[k] for k in ('sp', 'pk', 'part', 'loss_part'))     # the small state uses a part of each
    arena = Arena('cuda', band)
    bufs = {k: arena.take(k, (v,), F32, 'poison') for k, v in sizes.items()}
    for st in states:
        st._bind(bufs)
        st._arena_views = {}
        for t in (st.slab, st.loss_part, st.sp, st.pk, st.part):
            assert arena.holds(t)
    order = (0, 1) if first == 'large-first' else (1, 0)
    for k in order:
        got = one_epoch(eng, states[k], SHARED[k])
        arena.check()
        assert_no_poison(SHARED[k], got, f'shared scratch, {first}')
        assert_same_bits(SHARED[k], own[k], got, f'scratch of its own and the shared scratch ({first})')


# ------------------------------------------------------------------------------------------------------------------------
# the guard speaks
# ------------------------------------------------------------------------------------------------------------------------
def test_a_write_behind_sp_is_seen(eng, monkeypatch):
    """No kernel involved: one torch write of a float behind the re-homed sp, and check() names sp."""
    c = SHARED[1]
    st = build_state(eng, monkeypatch, c, problem_of(c))
    arena = Arena('cuda', NAN_BAND)
    views = rehome(st, arena)
    arena.check()
    sp = views['sp']
    assert st.sp.data_ptr() == sp.data_ptr() and st.sp.numel() == sp.numel() == c.m * c.S
    end = sp.data_ptr() - arena.buf.data_ptr() + sp.numel() * 4
    arena.buf[end:end + 4].view(F32)[0] = 1.0                                  # sp[m, S]: the element behind the last
    with pytest.raises(GuardDamaged, match="behind 'sp'"):
        arena.check()


# ------------------------------------------------------------------------------------------------------------------------
# the plan builders of the C ABI: outputs and a workspace of exactly *_workspace_bytes() in an arena
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('band', [NAN_BAND, BIG_BAND], ids=['nan', '2^60'])
def test_plan_builders_on_exact_workspaces(eng, monkeypatch, band):
    from teamoflow_amd import _lib
    lib, s, dev = _lib.get(), _lib.stream_ptr, 'cuda'
    c = next(x for x in CASES if x.id.startswith('wmrb-scores7fill'))
    p = problem_of(c)
    set_forms(monkeypatch, eng, c)
    m, n, S, r = c.m, c.n, c.S, c.r
    idx = torch.tensor(p['idx'][p['order']], device=dev)
    val = torch.tensor(p['val'][p['order']], device=dev)
    R = torch.tensor(p['R'], device=dev)
    nnz = idx.shape[0]
    plan = eng.InteractionPlan(idx, val, m, n, chunk=CHUNK)
    wplan = wmrb_plan(eng, plan, R, r, F32, True)
    s7 = eng.Scores7Plan(plan, wplan, r, F32, builder='device')
    C, i32, i64 = wplan.user_chunks, torch.int32, torch.int64
    arena = Arena(dev, band)

    def ws(name, nbytes):
        assert nbytes > 0
        return arena.take(name, (nbytes,), torch.uint8), nbytes

    def done():
        torch.cuda.synchronize()
        arena.check()

    # tmf_csr_build
    rowptr_u, col_u, val_u, user_of = (arena.take('rowptr_u', (m + 1,), i64), arena.take('col_u', (nnz,), i32), arena.take('val_u', (nnz,), F32),
                                       arena.take('user_of', (nnz,), i32))
    _lib.check(lib.tmf_csr_build(idx.contiguous(), val, nnz, m, n, rowptr_u, col_u, val_u, user_of, *ws('csr_ws', lib.tmf_csr_build_workspace_bytes(nnz)), s()), lib)
    done()
    assert torch.equal(rowptr_u, plan.rowptr_u) and torch.equal(col_u, plan.col_u) and torch.equal(val_u, plan.val_u) and torch.equal(user_of, plan.user_of)
    # tmf_csc_perm
    rowptr_i, perm = arena.take('rowptr_i', (n + 1,), i64), arena.take('perm_i', (nnz,), i64)
    _lib.check(lib.tmf_csc_perm(col_u, nnz, n, rowptr_i, perm, *ws('csc_ws', lib.tmf_stable_order_workspace_bytes(nnz)), s()), lib)
    done()
    assert plan.user_chunks == 1 and torch.equal(rowptr_i, plan.rowptr_i) and torch.equal(user_of[perm], plan.row_i) and torch.equal(val_u[perm], plan.val_i)
    # tmf_stable_order_i32, with and without the sorted keys
    keys = (torch.arange(nnz, device=dev) * 7919 % 37).to(i32)
    want_perm, want_rowptr = eng.stable_order(keys, 37)
    for with_keys in (False, True):
        perm2, rowptr2 = arena.take(f'perm_{with_keys}', (nnz,), i64), arena.take(f'rowptr_{with_keys}', (38,), i64)
        sorted_keys = arena.take('sorted_keys', (nnz,), i32) if with_keys else None
        _lib.check(lib.tmf_stable_order_i32(keys, nnz, 37, perm2, sorted_keys, rowptr2, *ws(f'order_ws_{with_keys}', lib.tmf_stable_order_workspace_bytes(nnz)), s()), lib)
        done()
        assert torch.equal(perm2, want_perm) and torch.equal(rowptr2, want_rowptr)
        assert sorted_keys is None or torch.equal(sorted_keys, keys[want_perm])
    # tmf_sort_samples
    Rs = arena.take('R_sorted', (m, S), i32)
    _lib.check(lib.tmf_sort_samples(R, m, S, n, Rs, *ws('sort_ws', lib.tmf_sort_samples_workspace_bytes(m, S)), s()), lib)
    done()
    assert wplan.sliced and torch.equal(Rs, wplan.R)
    # tmf_wmrb_entry_lists
    E = nnz + m * S
    ent_row, ent_id, rowptr_e = arena.take('ent_row', (E,), i32), arena.take('ent_id', (E,), i32), arena.take('rowptr_e', (C * n + 2,), i64)
    _lib.check(lib.tmf_wmrb_entry_lists(user_of, col_u, val_u, nnz, Rs, m, S, n, C, ent_row, ent_id, rowptr_e,
                                        *ws('lists_ws', lib.tmf_wmrb_entry_lists_workspace_bytes(nnz, m, S)), s()), lib)
    done()
    assert C > 1 and torch.equal(ent_row, wplan.ent_row) and torch.equal(ent_id, wplan.ent_w) and torch.equal(rowptr_e[:C * n + 1], wplan.rowptr_e)
    # tmf_s7plan_chunks / _subs / _streams
    nc = s7.n_slices * s7.n_groups
    head = (rowptr_u, col_u, Rs, nnz, m, S, n, s7.width, s7.slots)
    chunk_ent, chunk_sub = arena.take('chunk_ent', (nc + 1,), i64), arena.take('chunk_sub', (nc + 1,), i32)
    _lib.check(lib.tmf_s7plan_chunks(*head, chunk_ent, chunk_sub, *ws('chunks_ws', lib.tmf_s7plan_workspace_bytes(nc)), s()), lib)
    done()
    assert nc > 1 and torch.equal(chunk_sub, s7.chunk_sub) and torch.equal(chunk_ent, s7._dev[3])
    n_sub = int(chunk_sub[-1])
    sub_fill, sub_place, sub_step = arena.take('sub_fill', (n_sub, 4), i32), arena.take('sub_place', (n_sub + 1,), i64), arena.take('sub_step', (n_sub + 1,), i64)
    _lib.check(lib.tmf_s7plan_subs(*head, chunk_ent, chunk_sub, n_sub, sub_fill, sub_place, sub_step, *ws('subs_ws', lib.tmf_s7plan_workspace_bytes(n_sub)), s()), lib)
    done()
    assert n_sub == s7.n_sub and torch.equal(sub_place, s7.sub_place) and torch.equal(sub_step, s7.sub_step) and torch.equal(sub_fill, s7._dev[4])
    n_steps = int(sub_step[-1])
    assert n_steps == s7.n_steps
    for fill_order in (0, 1):
        steps, place = arena.take(f'steps_{fill_order}', (n_steps + 1, 4), i32), arena.take(f'place_{fill_order}', (E,), i32)
        _lib.check(lib.tmf_s7plan_streams(*head, chunk_ent, chunk_sub, n_sub, sub_step, n_steps, fill_order, steps, place, s()), lib)
        done()
        if fill_order:
            s7.order_by_fill()
        assert torch.equal(steps, s7.steps) and torch.equal(place, s7.place), fill_order
