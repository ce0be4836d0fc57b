"""The generated reduce kernels and the two finalize kernels on a real MI355X,
skeleton by skeleton and path by path (tests/reduce_ref.py holds the cases,
the data and NumPy's answers; tests/test_reduce_ref.py checks those on the CPU).

(a) paths -- every case of reduce_ref.CASES calls HipBackend.reduce on a
    backend of its own, on views into NaN / sentinel-filled buffers, and first
    asserts the path it was written for (reduce_ref.check_plan on the single
    entry of _reduce_plans, the single 'reduce' key of _sig_fns, the grid),
    then compares every output with NumPy: sums of integer-valued data are
    exact in any order, min / max / argmin / argmax run on extremes, ties and
    NaNs planted where the plan that really ran can go wrong.
(b) spx_reduce_finalize and spx_argreduce_combine called directly, both
    finalize kernels, against a plain NumPy fold.

Every number is exact by construction; the one tolerance is the a-priori
bound n eps sum|v| of test_float_sum_accuracy.
"""
import numpy as np
import pytest

import map_ref
import reduce_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture
def red(gpu_ctx):
  """A HipBackend of this test's own whose launches are recorded (launch_log);
  _reduce_plans and _sig_fns are emptied before every call (_reduce)."""
  from spartan_amd import backend
  be = backend.HipBackend()
  be.launch_log = []
  return be


def _view(vals, form, V, fill):
  """A device view holding ``vals`` inside a buffer of ``fill``: a lead before
  it, a pad after every innermost row, a tail after the last row
  (reduce_ref.layout)."""
  import torch
  from spartan_amd import backend
  vals = np.asarray(vals)
  lay = R.layout(form, vals.shape, V)
  buf = torch.full((lay.total,), fill, dtype=backend.torch_dtype(vals.dtype), device='cuda')
  v = torch.as_strided(buf, tuple(vals.shape), lay.strides, lay.lead)
  v.copy_(torch.from_numpy(np.ascontiguousarray(vals)))
  return v


def _reduce(be, case, root, op, ins, shape, odt, geom=None):
  """One HipBackend.reduce; the path assertions; (host result, plan)."""
  be._reduce_plans.clear()
  be._sig_fns.clear()
  del be.launch_log[:]
  _, _, outer, inner = R.seg_shape(shape, case.axis)
  got = be.reduce(root, op, ins, shape, case.axis, outer + inner, odt, geom)
  (entry,) = be._reduce_plans.values()
  plan = entry[0]
  (key,) = [k for k in be._sig_fns if k[0] == 'reduce']
  assert key[1] == root.sig() and key[5] == op
  assert (key[3], key[4], key[6], key[7], key[8]) == (plan.classes, plan.kind, plan.V, plan.U, plan.rowinv)
  R.check_plan(case, plan)
  narrowed = np.dtype(odt) in R.NARROW  # the result's narrowing cast is a map launch of its own
  assert be.launch_log[:1] == [plan.nblk] and len(be.launch_log) == (2 if narrowed else 1), (be.launch_log, plan.nblk)
  if op in ('argmin', 'argmax'):
    return (got[0].cpu().numpy(), got[1].cpu().numpy()), plan
  return got.cpu().numpy(), plan


def _compare(got, want, op, label):
  from spartan_amd import codegen
  if op in ('argmin', 'argmax'):
    (gv, gi), (wv, wi) = got, want
    assert gi.dtype == np.int64
    np.testing.assert_array_equal(gi, wi.reshape(gi.shape), err_msg=label + ' (indices)')
    assert gv.dtype == codegen.acc_dtype(op, wv.dtype), (label, gv.dtype)
    np.testing.assert_array_equal(gv, wv.reshape(gv.shape).astype(gv.dtype), err_msg=label + ' (values)')
  else:
    assert got.dtype == want.dtype, (label, got.dtype, want.dtype)
    np.testing.assert_array_equal(got, want.reshape(got.shape), err_msg=label)


def _operands(case, dt, op, vals):
  V = R.case_v(dt, op)
  host = R.case_operands(case, dt, vals)
  return {k: _view(h, form, V, R.fill_value(dt, op)) for k, (h, (form, _)) in enumerate(zip(host, case.operands))}


def _run_case(be, case, dt):
  """Every op of the case on ``dt``: the sum on reduce_ref.values, min / max /
  arg ops first on the same values (which gives the plan that really runs)
  and then on every planted scenario of that plan's geometry."""
  root = R.case_root(case, dt)
  ops = R.case_ops(case, dt)
  assert ops
  own = len(case.operands) == 1
  if 'sum' in ops:
    shape = R.case_shape(case, dt, 'sum')
    vals = R.values(shape, case.axis, dt, span=R.IL_BIG_SPAN if case is R.IL_BIG else None)
    got, _ = _reduce(be, case, root, 'sum', _operands(case, dt, 'sum', vals), shape, R.out_dtype('sum', dt))
    _compare(got, R.expected(vals, 'sum', case.axis, R.out_dtype('sum', dt)), 'sum', '%s sum %s' % (case.name, dt))
  for side, pair in (('lo', ('min', 'argmin')), ('hi', ('max', 'argmax'))):
    mine = [op for op in pair if op in ops]
    if not mine:
      continue
    shape = R.case_shape(case, dt, mine[0])
    nseg, n, _, _ = R.seg_shape(shape, case.axis)
    seg = R.seg_values(nseg, n, R.span_for(dt))
    vals = R.from_segments(R.to_dtype(seg, dt), shape, case.axis)
    ins = _operands(case, dt, mine[0], vals)
    plan = None
    for op in mine:
      got, plan = _reduce(be, case, root, op, ins, shape, R.out_dtype(op, dt))
      _compare(got, R.expected(vals, op, case.axis, R.out_dtype(op, dt)), op, '%s %s %s' % (case.name, op, dt))
    scen = R.scenarios(dt, R.edge_positions(**R.geometry(plan)))
    for rnd in range(0, len(scen), nseg):
      vals = R.from_segments(R.plant(seg, dt, side, scen, rnd, own), shape, case.axis)
      ins = _operands(case, dt, mine[0], vals)
      for op in mine:
        got, _ = _reduce(be, case, root, op, ins, shape, R.out_dtype(op, dt))
        _compare(got, R.expected(vals, op, case.axis, R.out_dtype(op, dt)), op,
                 '%s %s %s, scenarios %s from segment %d on' % (case.name, op, dt, [s[0] for s in scen], -rnd % len(scen)))


def _params(cases):
  pairs = [(c, dt) for c in cases for dt in c.dts]
  return dict(argnames='case,dt', argvalues=pairs, ids=['%s-%s' % (c.name, dt.name) for c, dt in pairs])


# ------------------------------------------------------------------ (a) paths
@pytest.mark.parametrize(**_params(R.CASES))
def test_path(red, case, dt):
  _run_case(red, case, dt)


@pytest.mark.parametrize(**_params(R.NARROW_CASES))
def test_narrow_integers(red, case, dt):
  """int8 / uint8 / int16 through the three skeletons, with P == 1 and P > 1:
  min / max / arg ops accumulate in int32, the result is narrowed by the
  identity-cast map (a sum wraps like astype)."""
  _run_case(red, case, dt)


@pytest.mark.parametrize(**_params(R.IL_CASES))
def test_cols_interleaved(red, monkeypatch, case, dt):
  from spartan_amd import backend
  monkeypatch.setattr(backend, 'COLS_INTERLEAVE', True)
  _run_case(red, case, dt)


def test_cols_interleaved_middle_sum(red, monkeypatch):
  """One block per CU and enough rows that a block walks more than 32
  super-chunks plus a remainder: the middle sum is folded into the total at
  least once and the rest at the end."""
  from spartan_amd import backend
  monkeypatch.setattr(backend, 'COLS_INTERLEAVE', True)
  monkeypatch.setattr(backend, 'COLS_BLOCKS_PER_CU', 1)
  _run_case(red, R.IL_BIG, R.F32)


def _geom_case(kind):
  return {'rowsp': R.make_case('geom-rowsp', (R.F32,), (37, 36), 1, 'rowsp', True),
          'rows': R.make_case('geom-rows', (R.F32,), (3, 4100), 1, 'rows', True, ('P>1',)),
          'cols': R.make_case('geom-cols', (R.F32,), (300, 260), 0, 'cols', True, ('P>1', 'CT>1'), U=4)}[kind]


@pytest.mark.parametrize('dt', [R.F32, R.I64], ids=lambda d: d.name)
@pytest.mark.parametrize('kind', ['rowsp', 'rows', 'cols'])
def test_arg_index_offset(red, kind, dt):
  """idx_geom offset k: the tile's place along the reduced axis is added to
  every index (and not to the empty marker of lanes without an element)."""
  case = _geom_case(kind)
  shape = case.shape
  for op, side in (('argmin', 'lo'), ('argmax', 'hi')):
    nseg, n, _, _ = R.seg_shape(shape, case.axis)
    seg = R.seg_values(nseg, n)
    plan = R.host_plan(case, dt, op)
    scen = R.scenarios(dt, R.edge_positions(**R.geometry(plan)))
    vals = R.from_segments(R.plant(seg, dt, side, scen), shape, case.axis)
    got, _ = _reduce(red, case, R.case_root(case, dt), op, _operands(case, dt, op, vals), shape, R.I64,
                     {'offset': 123456789012})
    wv, wi = R.expected(vals, op, case.axis, R.I64)
    _compare(got, (wv, wi + 123456789012), op, '%s %s offset' % (case.name, op))


@pytest.mark.parametrize('dt', [R.F32, R.I64], ids=lambda d: d.name)
@pytest.mark.parametrize('kind,tshape', [('rowsp', (2, 5, 6)), ('rows', (4, 50, 60))])
def test_arg_index_decompose(red, kind, tshape, dt):
  """axis None over a tile that is no run of whole rows of its array: the flat
  tile index is unravelled in the tile, shifted by the tile's corner and
  ravelled in the array."""
  tul, ashape = (4, 0, 10), (16, tshape[1], 100)
  geom = {'decompose': True, 'tshape': tshape, 'tul': tul, 'ashape': ashape}
  case = R.make_case('geom-flat-' + kind, (dt,), tshape, None, kind, True, ('P>1',) if kind == 'rows' else (),
              [('flat', None)])
  for op, side in (('argmin', 'lo'), ('argmax', 'hi')):
    n = int(np.prod(tshape))
    plan = R.host_plan(case, dt, op, geom=geom)
    scen = R.scenarios(dt, R.edge_positions(**R.geometry(plan)))
    for rnd in range(len(scen)):
      vals = R.plant(R.seg_values(1, n), dt, side, scen, rnd).reshape(tshape)
      got, _ = _reduce(red, case, R.case_root(case, dt), op, _operands(case, dt, op, vals), tshape, R.I64, geom)
      wv, wi = R.expected(vals, op, None, R.I64)
      loc = np.unravel_index(int(wi), tshape)
      want = np.ravel_multi_index(tuple(x + u for x, u in zip(loc, tul)), ashape)
      _compare(got, (wv, np.asarray(want, dtype=np.int64)), op, '%s %s %s' % (case.name, op, scen[rnd % len(scen)]))


@pytest.mark.parametrize('dt', R.NARROW, ids=lambda d: d.name)
def test_narrow_integers_through_the_expr_api(gpu_ctx, dt):
  """A map into int8 / uint8 / int16 followed by a reduction: what the expr
  layer asks of backend.reduce (the value type as the result type, a sum
  wrapping like astype)."""
  from spartan_amd import expr
  lo = 0 if dt.kind == 'u' else 50
  host = ((np.arange(37 * 144, dtype=np.int64) * 37) % 100 - lo).reshape(37, 144).astype(dt)
  x = expr.astype((expr.arange((37, 144), dtype=np.int64) * 37) % 100 - lo, dt)
  for name in ('max', 'min', 'sum', 'argmin', 'argmax'):
    for axis in (0, 1, None):
      got = getattr(expr, name)(x, axis=axis).glom()
      if name == 'sum':
        want = host.astype(np.int64).sum(axis=axis).astype(dt)
      else:
        want = getattr(np, name)(host, axis=axis)
      assert np.asarray(got).dtype == np.asarray(want).dtype, (name, axis, np.asarray(got).dtype)
      np.testing.assert_array_equal(got, want, err_msg='%s axis %s %s' % (name, axis, dt))


_MIXED = [R.make_case('mixed-rowsp', (R.F64,), (37, 18), 1, 'rowsp', True, ('lanes=16',), [('c', None)] * 2),
          R.make_case('mixed-rows', (R.F64,), (3, 2052), 1, 'rows', True, ('P==2',), [('c', None)] * 2),
          R.make_case('mixed-cols', (R.F64,), (300, 130), 0, 'cols', True, ('CT==2', 'P>1'), [('c', None)] * 2)]


@pytest.mark.parametrize('case', _MIXED, ids=[c.name for c in _MIXED])
def test_mixed_item_sizes(red, case):
  """int8 + float64: V = 2 (the widest item decides), the int8 operand is
  loaded two elements at a time."""
  from spartan_amd.codegen import In, Op
  root = Op('add', [In(0, R.I8), In(1, R.F64)])
  shape = case.shape
  nseg, n, _, _ = R.seg_shape(shape, case.axis)
  x0 = R.small_operand(shape, R.I8, 5)
  for op, side in (('sum', None), ('min', 'lo'), ('argmax', 'hi')):
    seg = R.seg_values(nseg, n)
    if side:
      plan = R.host_plan(case, R.F64, op, in_dts=[R.I8, R.F64])
      seg = R.plant(seg, R.F64, side, R.scenarios(R.F64, R.edge_positions(**R.geometry(plan))))
    vals = R.from_segments(seg.astype(R.F64), shape, case.axis)
    with np.errstate(all='ignore'):
      x1 = vals - x0
    ins = {0: _view(x0, 'c', 2, R.fill_value(R.I8, op)), 1: _view(x1, 'c', 2, np.nan)}
    got, plan = _reduce(red, case, root, op, ins, shape, R.out_dtype(op, R.F64))
    assert plan.V == 2
    _compare(got, R.expected(vals, op, case.axis, R.out_dtype(op, R.F64)), op, '%s %s' % (case.name, op))


_BOOL = [R.make_case('bool-rowsp', (R.B,), (37, 18), 1, 'rowsp', True, ('lanes=16',)),
         R.make_case('bool-rows', (R.B,), (3, 2052), 1, 'rows', True, ('P==2',)),
         R.make_case('bool-cols', (R.B,), (300, 130), 0, 'cols', True, ('CT==2', 'P>1'), U=4)]


@pytest.mark.parametrize('case', _BOOL, ids=[c.name for c in _BOOL])
def test_bool_sum(red, case):
  """A bool sum counts in an int64 accumulator (V = 2, bools loaded in pairs)."""
  from spartan_amd.codegen import In
  shape = case.shape
  nseg, n, _, _ = R.seg_shape(shape, case.axis)
  vals = R.from_segments(R.seg_values(nseg, n) % 3 == 0, shape, case.axis)
  # the sentinel around the view is True: a stray read counts
  got, plan = _reduce(red, case, In(0, R.B), 'sum', {0: _view(vals, 'c', 2, True)}, shape, R.I64)
  assert plan.V == 2 and plan.pdt == R.I64
  _compare(got, R.expected(vals, 'sum', case.axis, R.I64), 'sum', case.name)


@pytest.mark.parametrize('op', R.OPS)
def test_empty_output_launches_nothing(red, op):
  import torch
  from spartan_amd.codegen import In
  x = torch.empty((0, 5), dtype=torch.float32, device='cuda')
  got = red.reduce(In(0, R.F32), op, {0: x}, (0, 5), 1, (0,), R.out_dtype(op, R.F32))
  assert red.launch_log == [] and not red._sig_fns
  for t in (got if isinstance(got, tuple) else (got,)):
    assert tuple(t.shape) == (0,)


_ACC = [(n, dt) for n in ('rowsp-R9V', 'rows-two-chunks', 'cols-outer-partials') for dt in (R.F32, R.F64)]


@pytest.mark.parametrize('name,dt', _ACC, ids=['%s-%s' % (n, d.name) for n, d in _ACC])
def test_float_sum_accuracy(red, name, dt):
  """Decimal (not integer-valued) data: the sum may differ from the
  long-double sum by the rounding of another summation order, at most
  n eps sum|v| -- the a-priori bound of recursive summation in any order
  (derived, not measured)."""
  (case,) = [c for c in R.CASES if c.name == name]
  shape = R.case_shape(case, dt, 'sum')
  grid = map_ref.decimal_grid(dt)[0]
  vals = grid[(np.arange(int(np.prod(shape))) * 7) % len(grid)].reshape(shape)
  got, _ = _reduce(red, case, R.case_root(case, dt), 'sum', {0: _view(vals, 'c', R.case_v(dt, 'sum'), np.nan)}, shape, dt)
  n = shape[case.axis]
  tol = n * np.finfo(dt).eps * np.sum(np.abs(vals.astype(np.float64)), axis=case.axis)
  err = np.abs(got.astype(np.longdouble) - np.sum(vals.astype(np.longdouble), axis=case.axis))
  print('REDUCE_SUM_ERR %s %s max err / bound = %.3g' % (name, dt.name, float(np.max(err / tol))))
  assert (err <= tol).all()


# ------------------------------------------- (b) finalize and arg-combine
FIN_P = [1, 2, 31, 32, 33, 255, 256, 257, 600]
FIN_N = [1, 3, 16384, 16385]   # 16385: P >= 32 goes back to the narrow kernel
FIN_TYPES = [(R.F32, R.F32), (R.F64, R.F32), (R.F64, R.F64), (R.I64, R.I64), (R.I64, R.I32)]


def _dev(a):
  import torch
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _partials(P, n, dt):
  """(P, n) integer-valued partials; int64 ones large enough that their sum
  (and min / max) wraps in an int32 result."""
  base = R.seg_values(n, P, salt=P).T
  if np.dtype(dt) == R.I64:
    return base * (1 << 29) + np.arange(P, dtype=np.int64)[:, None]
  return base.astype(dt)


@pytest.mark.parametrize('P', FIN_P)
def test_finalize(red, P):
  import torch
  from spartan_amd import backend
  for n in FIN_N:
    for pdt in (R.F32, R.F64, R.I64):
      parts = _partials(P, n, pdt)
      variants = [parts]
      if pdt.kind == 'f':  # min / max: a NaN in the first, a middle and the last partial
        nanned = parts.copy()
        for k, p in enumerate((0, P // 2, P - 1)):
          nanned[p, k % n] = np.nan
        variants.append(nanned)
      for vi, host in enumerate(variants):
        dev = _dev(host.reshape(-1))
        for odt in [o for q, o in FIN_TYPES if q == pdt]:
          for op in ('sum', 'min', 'max'):
            if vi == 1 and op == 'sum':
              continue
            out = torch.full((n,), 77, dtype=backend.torch_dtype(odt), device='cuda')
            red.finalize(op, dev, P, n, out)
            with np.errstate(all='ignore'):
              want = R.fold(op, host).astype(odt)
            np.testing.assert_array_equal(out.cpu().numpy(), want,
                                          err_msg='finalize %s P %d n %d %s -> %s%s' % (op, P, n, pdt, odt, ' NaN' * vi))
  assert red.launch_log == []  # ahead-of-time kernels only


def _arg_layout(rng, P, n):
  """What the (values, indices) partials of one (P, n) share: indices distinct
  per column and not monotonic in p, a few distinct small values (ties in
  several partials), a third of the slots empty, one column (of several) all
  empty, and where the float variants hold a NaN (in a quarter of the columns)."""
  m = 7 if P % 7 else 11
  assert P % m
  idx = ((np.arange(P, dtype=np.int64)[:, None] * m + np.arange(n, dtype=np.int64)[None, :]) % P) * 3 + 5
  small = rng.integers(-1, 2, size=(P, n))
  empty = rng.random((P, n)) < 1 / 3
  if n > 1:
    empty[:, n // 2] = True
  nans = (rng.random((P, n)) < 0.3) & (rng.random(n) < 0.25)[None, :]
  idx[empty] = R.EMPTY
  return idx, small, empty, nans


def _arg_partials(lay, dt, op):
  """(values, indices) in ``dt``: int64 values lie around 2^60; an empty slot
  holds the value that would win."""
  idx, small, empty, nans = lay
  if np.dtype(dt).kind == 'i':
    vals = ((np.int64(1) << 60 if dt == R.I64 else 0) + small).astype(dt)
    win = vals.min() - 1 if op == 'argmin' else vals.max() + 1
  else:
    vals = small.astype(dt)
    vals[nans] = np.nan
    win = -np.inf if op == 'argmin' else np.inf
  vals[empty] = win
  return vals, idx


def _check_arg(got_v, got_i, host_v, host_i, op, label):
  wv, wi = R.arg_fold(op, host_v, host_i)
  np.testing.assert_array_equal(got_i, wi, err_msg=label + ' (indices)')
  live = wi != R.EMPTY  # an all-empty column has no value
  assert (~live).any() or host_v.shape[1] == 1
  np.testing.assert_array_equal(got_v[live], wv[live], err_msg=label + ' (values)')


@pytest.mark.parametrize('P', FIN_P)
def test_finalize_arg(red, P):
  import torch
  from spartan_amd import backend
  rng = np.random.default_rng(P)
  for n in FIN_N:
    lay = _arg_layout(rng, P, n)
    for dt in (R.F32, R.F64, R.I64):
      for op in ('argmin', 'argmax'):
        hv, hi = _arg_partials(lay, dt, op)
        out_i = torch.full((n,), -7, dtype=torch.int64, device='cuda')
        out_v = torch.full((n,), 77, dtype=backend.torch_dtype(dt), device='cuda')
        red._finalize(op, dt, np.int64, _dev(hv.reshape(-1)), _dev(hi.reshape(-1)), P, n, out_i, out_v)
        _check_arg(out_v.cpu().numpy(), out_i.cpu().numpy(), hv, hi, op, '_finalize %s P %d n %d %s' % (op, P, n, dt))


@pytest.mark.parametrize('dt', [R.F32, R.F64, R.I32, R.I64], ids=lambda d: d.name)
def test_argcombine(red, dt):
  rng = np.random.default_rng(11)
  for Rr in (1, 2, 5, 33):
    for n in (1, 3, 1000):
      lay = _arg_layout(rng, Rr, n)
      for op in ('argmin', 'argmax'):
        hv, hi = _arg_partials(lay, dt, op)
        gv, gi = red.argcombine(op, _dev(hv), _dev(hi))
        assert gv.dtype == _dev(hv).dtype and tuple(gi.shape) == (n,)
        _check_arg(gv.cpu().numpy(), gi.cpu().numpy(), hv, hi, op, 'argcombine %s R %d n %d %s' % (op, Rr, n, dt))
