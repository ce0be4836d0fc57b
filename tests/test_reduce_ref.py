"""CPU self-checks of tests/reduce_ref.py: the data holds the properties the
GPU comparison rests on (integer-valued, non-zero, distinct within a window,
sums exact in any order for every listed shape), the planted scenarios put
NumPy's answer where they claim, every case's path expectation holds for
backend.plan_reduce at 256 CUs, and a case whose plan is moved off its path
fails with its "written for" message."""
import numpy as np
import pytest

import reduce_ref as R
from spartan_amd import backend

ALL_CASES = R.CASES + R.NARROW_CASES + R.IL_CASES + [R.IL_BIG]
_PAIRS = [(c, dt) for c in ALL_CASES for dt in c.dts]
_IDS = ['%s-%s' % (c.name, dt.name) for c, dt in _PAIRS]


def test_case_names_are_unique():
  names = [c.name for c in ALL_CASES]
  assert len(names) == len(set(names))


@pytest.mark.parametrize('span', [60, R.SPAN])
def test_values_nonzero_and_distinct_in_every_window(span):
  seg = R.seg_values(7, 5 * span + 3, span)
  assert (seg != 0).all() and np.abs(seg).max() == span
  W = 2 * span
  for s in range(seg.shape[0]):
    for r0 in (0, 1, span, seg.shape[1] - W):
      assert len(set(seg[s, r0:r0 + W])) == W
  assert not (seg[0] == seg[1]).all()  # segments differ


@pytest.mark.parametrize('dt', R.MAIN + R.NARROW, ids=lambda d: d.name)
def test_values_are_the_same_integers_in_every_dtype(dt):
  v = R.values((5, 300), 1, dt)
  ref = R.seg_values(5, 300, R.span_for(dt))
  if dt.kind == 'u':
    ref = ref + R.span_for(dt) + 1
  np.testing.assert_array_equal(v.astype(np.int64), ref)
  assert (v != 0).all()
  # segments follow the reduced axis
  np.testing.assert_array_equal(R.values((300, 5), 0, dt), v.T)
  np.testing.assert_array_equal(R.values((2, 300, 3), 1, dt)[1, :, 2], R.from_segments(R.to_dtype(
      R.seg_values(6, 300, R.span_for(dt)), dt), (2, 300, 3), 1)[1, :, 2])


@pytest.mark.parametrize('case,dt', _PAIRS, ids=_IDS)
def test_sums_are_exact_in_any_order(case, dt):
  """The partial-sum bound: sum |v| over a segment (hence every partial sum of
  absolute values) is below 2^24 / 2^53 / 2^63."""
  assert R.case_ops(case, dt)
  shape = max((R.case_shape(case, dt, op) for op in R.case_ops(case, dt)), key=np.prod)
  nseg, n, _, _ = R.seg_shape(shape, case.axis)
  span = R.IL_BIG_SPAN if case is R.IL_BIG else R.span_for(dt)
  worst = span + (R.span_for(dt) if dt.kind == 'u' else 0) + 1
  assert n * worst < R.exact_limit(dt)
  if nseg * n <= 1 << 20:
    seg = R.seg_values(nseg, n, span)
    assert np.abs(seg).sum(axis=1).max() < R.exact_limit(dt)


@pytest.mark.parametrize('case,dt', _PAIRS, ids=_IDS)
def test_every_case_is_on_its_path_at_256_cus(monkeypatch, case, dt):
  if case in R.IL_CASES or case is R.IL_BIG:
    monkeypatch.setattr(backend, 'COLS_INTERLEAVE', True)
  if case is R.IL_BIG:
    monkeypatch.setattr(backend, 'COLS_BLOCKS_PER_CU', 1)
  for op in R.case_ops(case, dt):
    R.check_plan(case, R.host_plan(case, dt, op))


def _case(name):
  (c,) = [c for c in ALL_CASES if c.name == name]
  return c


@pytest.mark.parametrize('name,knob,value', [
    ('rows-capped', 'ROWS_GRID_PER_CU', 1 << 20),   # no cap: a block per segment
    ('cols-2-tiles', 'COLS_BLOCKS_PER_CU', 0),      # no partial chunks
    ('rowsp-R9V', '_lanes', lambda need: 64),       # another lane-group width
])
def test_a_case_off_its_path_says_so(monkeypatch, name, knob, value):
  case = _case(name)
  R.check_plan(case, R.host_plan(case, R.F32, 'sum'))
  monkeypatch.setattr(backend, knob, value)
  with pytest.raises(AssertionError, match='case %s: plan .* this case was written for' % name):
    R.check_plan(case, R.host_plan(case, R.F32, 'sum'))


def test_a_case_on_another_skeleton_or_path_says_so():
  case = _case('rows-two-chunks')
  other = R.host_plan(_case('rowsp-R9V'), R.F32, 'sum')
  with pytest.raises(AssertionError, match='this case was written for'):
    R.check_plan(case, other)
  with pytest.raises(AssertionError, match='this case was written for'):
    R.check_plan(case, R.host_plan(_case('rows-two-chunks-offset'), R.F32, 'sum'))


@pytest.mark.parametrize('case,dt', [(c, c.dts[0]) for c in R.CASES], ids=[c.name for c in R.CASES])
def test_edge_positions_lie_in_the_segment(case, dt):
  plan = R.host_plan(case, dt, 'min')
  g = R.geometry(plan)
  pos = R.edge_positions(**g)
  assert {'first', 'last', 'last_lane', 'tail_loop'} <= set(pos)
  assert ('chunk_boundary' in pos) == (plan.P > 1)
  for name, ps in pos.items():
    assert ps and all(0 <= p < g['R'] for p in ps), (name, ps)
  if plan.P > 1:
    a, b = pos['chunk_boundary']
    assert a // g['chunk'] + 1 == b // g['chunk']  # last of chunk p, first of chunk p + 1
  if plan.kind == 'rows' and g['U'] > 1:
    # lane 0's unrolled loop (r + (U - 1) * 256 V < r1) has ended at the tail position
    (t,) = pos['tail_loop']
    step = 256 * g['per']
    clen = min(g['chunk'], g['R'])
    assert t == clen - 1 or (t % (g['U'] * step) == 0 and t + (g['U'] - 1) * step >= clen)


@pytest.mark.parametrize('dt', [R.F32, R.I32, R.I8, R.U8], ids=lambda d: d.name)
def test_planted_scenarios_are_what_numpy_sees(dt):
  pos = {'first': [0], 'last': [99], 'pair': [40, 41], 'far': [63, 64]}
  scen = R.scenarios(dt, pos)
  seg = R.seg_values(len(scen), 100, R.span_for(dt))
  for side, op in (('lo', 'argmin'), ('hi', 'argmax')):
    v = R.plant(seg, dt, side, scen)
    assert v.dtype == dt
    vals, idx = R.expected(v, op, 1, R.I64)
    for s, (what, ps) in enumerate(scen):
      if what in ('ext', 'nan'):
        assert idx[s] == ps[0], (what, ps)  # the first of a tie, the first NaN
        assert np.isnan(vals[s]) == (what == 'nan')
      else:
        assert idx[s] == 0
    if dt.kind != 'f':
      ii = np.iinfo(dt)
      assert set(np.unique(vals)) == ({ii.min, ii.min + (dt.kind == 'i')} if side == 'lo' else {ii.max, ii.max - 1})
  # another round rotates the scenarios over the segments
  v1 = R.plant(seg, dt, 'lo', scen, rnd=1)
  assert R.expected(v1, 'argmin', 1, R.I64)[1][0] == scen[1][1][0]


def test_multi_operand_values_are_exact():
  case = _case('cols-rowinv-b')
  shape = R.case_shape(case, R.F32, 'max')
  nseg, n, _, _ = R.seg_shape(shape, 0)
  scen = R.scenarios(R.F32, {'first': [0], 'pair': [10, 11]})
  vals = R.from_segments(R.plant(R.seg_values(nseg, n), R.F32, 'hi', scen, own=False), shape, 0)
  x = R.case_operands(case, R.F32, vals)
  assert [a.shape for a in x] == [(300, 260), (1, 260), (300, 1)]
  with np.errstate(all='ignore'):
    np.testing.assert_array_equal(x[0] + x[1] - x[2], vals)
  assert np.abs(x[0][np.isfinite(x[0])]).max() < 1 << 24


def test_fold_and_arg_fold_rules():
  nan = np.nan
  parts = np.array([[1.0, nan, 3.0], [2.0, 5.0, nan], [0.5, 7.0, 1.0]])
  np.testing.assert_array_equal(R.fold('min', parts), [0.5, nan, nan])
  np.testing.assert_array_equal(R.fold('sum', parts[:, :1]), [3.5])
  vals = np.array([[4.0, 4.0, nan, 9.0], [4.0, 1.0, nan, 0.0], [4.0, 1.0, 0.0, 0.0]])
  idx = np.array([[7, 3, 9, R.EMPTY], [2, 8, 4, R.EMPTY], [5, 6, 1, R.EMPTY]], dtype=np.int64)
  bv, bi = R.arg_fold('argmin', vals, idx)
  np.testing.assert_array_equal(bi, [2, 6, 4, R.EMPTY])
  np.testing.assert_array_equal(bv[:2], [4.0, 1.0])
  assert np.isnan(bv[2])
  big = np.array([[1 << 60], [(1 << 60) + 1], [(1 << 60) - 1]], dtype=np.int64)
  bv, bi = R.arg_fold('argmax', big, np.array([[0], [1], [2]], dtype=np.int64))
  assert (bv[0], bi[0]) == ((1 << 60) + 1, 1)


def test_layouts_keep_the_operand_inside_its_buffer():
  for form in R.FORMS:
    for shape in ((37, 36), (1, 8200)) + (() if form == 'T' else ((5, 7, 12),)):
      lay = R.layout(form, shape, 4)
      last = lay.lead + sum((s - 1) * st for s, st in zip(shape, lay.strides))
      assert lay.lead >= 16 and last + 16 < lay.total  # a lead before, a tail after
  assert R.layout('off', (3, 8), 4).lead % 4 == 1
  assert R.layout('pitch', (3, 8), 4).strides[0] % 4 == 1
  assert R.layout('T', (3, 8), 4).strides == (1, 8)
