"""Host checks of tests/map_ref.py, the reference of the generated map kernels:
its table covers every lowering of codegen.Emitter.op_expr, its inputs hold
the operands that separate the lowerings from near misses, and its expected
values agree with the test double's eval_ir.  No GPU."""
import inspect
import re

import numpy as np
import pytest

import map_ref as R
from fake_backend import eval_ir
from spartan_amd import codegen
from spartan_amd.codegen import Cast, In, Op, Sc


def lowered_names():
  """Every ufunc name op_expr tests ``name`` against, read from its source,
  with the keys of the two OCML tables."""
  src = inspect.getsource(codegen.Emitter.op_expr)
  names = set(re.findall(r"name == '(\w+)'", src))
  for group in re.findall(r"name in \(([^)]*)\)", src):
    names.update(re.findall(r"'(\w+)'", group))
  cmps = re.search(r"cmps = \{(.*?)\}", src, re.S).group(1)
  names.update(re.findall(r"'(\w+)':", cmps))
  return names | set(codegen.OCML_1) | set(codegen.OCML_2)


def _lower(op, dt):
  n = R.OPS[op]['arity']
  root = Op(op, [In(i, dt) for i in range(n)])
  codegen._expr_fn(root, [(i, dt) for i in range(n)])
  return root


def test_table_lists_every_lowering():
  names = lowered_names()
  assert len(names) >= 55 and {'add', 'floor_divide', 'greater_equal', 'isfinite', 'hypot', 'cbrt'} <= names
  assert names == set(R.OPS), 'lowered but not in map_ref.OPS: %s; listed but not lowered: %s' % (
      sorted(names - set(R.OPS)), sorted(set(R.OPS) - names))
  for op, t in R.OPS.items():
    assert getattr(np, op).nin == t['arity'], op


@pytest.mark.parametrize('op', sorted(R.OPS))
def test_dtypes_that_lower_are_the_table(op):
  """Each (op, dtype) of CANDIDATES either lowers and is in the table, or
  raises the codegen's documented TypeError / NotImplementedError."""
  for dt in R.CANDIDATES:
    if dt in R.OPS[op]['dtypes']:
      _lower(op, dt)
    else:
      with pytest.raises((TypeError, NotImplementedError)):
        _lower(op, dt)


def test_documented_refusals():
  with pytest.raises(TypeError, match='float16 not supported'):  # sqrt(int8) resolves to float16
    _lower('sqrt', R.I8)
  for dt in (np.uint16, np.uint32, np.uint64):
    with pytest.raises(TypeError, match='not supported by the gfx950 codegen'):
      _lower('add', np.dtype(dt))
  for op in ('floor', 'ceil', 'trunc'):
    with pytest.raises(NotImplementedError, match='no gfx950 lowering'):
      _lower(op, R.I32)
  with pytest.raises(NotImplementedError, match='no gfx950 lowering'):
    Op('fmod', [In(0, R.I32), In(1, R.I32)]) and _lower('fmod', R.I32)
  with pytest.raises(TypeError, match='no loop'):
    Op('negative', [In(0, R.B)])
  with pytest.raises(TypeError, match='no loop'):
    Op('subtract', [In(0, R.B), In(1, R.B)])


@pytest.mark.parametrize('dtype', R.SUPPORTED, ids=lambda d: d.name)
def test_specials(dtype):
  sp = R.specials(dtype)
  if dtype.kind == 'f':
    fi = np.finfo(dtype)
    assert len(sp) == 25 and np.isnan(sp[-1])
    for v in (0.0, 0.5, 1.5, 2.5, np.inf, fi.max, fi.tiny, fi.smallest_subnormal, dtype.type(np.pi / 2)):
      for s in (v, -v):
        assert np.any((sp == s) & (np.signbit(sp) == np.signbit(dtype.type(s)))), s
  elif dtype.kind == 'b':
    assert list(sp) == [False, True]
  else:
    ii = np.iinfo(dtype)
    assert {0, 1, 2, 3, 7, ii.min, ii.min + 1, ii.max - 1, ii.max} <= set(int(x) for x in sp)
    if dtype == R.I64:
      assert 2 ** 53 + 1 in sp and -(2 ** 53 + 1) in sp and int(float(2 ** 53 + 1)) != 2 ** 53 + 1


def test_inputs_are_fixed_and_complete():
  a, b = R.inputs('floor_divide', R.F32)
  a2, b2 = R._inputs.__wrapped__('floor_divide', R.F32)
  assert np.array_equal(R.bits(a), R.bits(a2)) and np.array_equal(R.bits(b), R.bits(b2))
  n_sp = len(R.specials(R.F32))
  assert len(a) == n_sp * n_sp + 101 * 38 + 2000 + 6
  for dt in R.FLOATS:  # the operands the issue names
    a, b = R.inputs('floor_divide', dt)
    for x, y in ((1.0, 0.1), (-1.0, np.inf)):
      assert np.any((a == dt.type(x)) & (b == dt.type(y))), (x, y)
  # (4, -2): a zero remainder of a negative divisor, from the decimal grid
  a, b = R.inputs('remainder', R.F64)
  with np.errstate(all='ignore'):
    z = (np.fmod(a, b) == 0) & (b < 0) & np.isfinite(a) & (a != 0)
  assert z.sum() > 50 and np.any((a == 4.0) & (b == -2.0))
  # integer power: no negative exponent; integer reciprocal: no zero
  for dt in R.INTS:
    assert (R.inputs('power', dt)[1] >= 0).all() and (R.inputs('reciprocal', dt)[0] != 0).all()
  a, b = R.inputs('floor_divide', R.I64)
  assert np.any((a == np.iinfo(np.int64).min) & (b == -1)) and np.any(b == 0)


@pytest.mark.parametrize('dt', R.FLOATS, ids=lambda d: d.name)
def test_inputs_separate_floor_divide_from_floor_of_quotient(dt):
  """The wrong lowering this reference was written against, floor(a / b), and
  fmod's unsigned zero differ from NumPy on these inputs (random normal draws
  alone never show it)."""
  a, b = R.inputs('floor_divide', dt)
  with np.errstate(all='ignore'):
    assert (R.bits(np.floor(a / b)) != R.bits(np.floor_divide(a, b))).sum() > 100
    assert np.floor_divide(dt.type(1.0), dt.type(0.1)) == 9 and np.floor(dt.type(1.0) / dt.type(0.1)) == 10
    r = np.fmod(a, b)
    old = np.where((r != 0) & ((r < 0) != (b < 0)), r + b, r)
    assert (R.bits(old) != R.bits(np.remainder(a, b))).sum() > 50


def _root(op, dt, scalar=None):
  if R.OPS[op]['arity'] == 1:
    return Op(op, [In(0, dt)])
  return Op(op, [In(0, dt), In(1, dt) if scalar is None else Sc(0, scalar)])


@pytest.mark.parametrize('op', sorted(R.OPS))
def test_expected_exact_agrees_with_eval_ir(op):
  """expected_exact (the ufunc on the arrays, scalars left weak) and the test
  double's IR evaluator (operands converted to the dtypes codegen.Op resolved)
  give the same bits on every (op, dtype), array and scalar form."""
  for dt in R.OPS[op]['dtypes']:
    args = R.inputs(op, dt)
    forms = [None] + (R.scalars(op, dt) if len(args) == 2 else [])
    for sc in forms:
      root = _root(op, dt, sc)
      call = args if sc is None else (args[0], sc)
      want = R.expected_exact(op, call)
      assert want.dtype == root.dtype, (op, dt, sc)
      got = np.asarray(eval_ir(root, dict(enumerate(args)), args[0].shape))
      np.testing.assert_array_equal(R.bits(got), R.bits(want), err_msg='%s %s scalar=%r' % (op, dt, sc))


def test_weak_scalars_keep_the_array_dtype():
  assert _root('add', R.F32, 1e-3).dtype == R.F32 and _root('multiply', R.I64, 2 ** 53 + 1).dtype == R.I64
  a = R.inputs('add', R.I64)[0]
  assert np.array_equal(R.expected_exact('add', (a[:4] * 0, 2 ** 53 + 1)), np.full(4, 2 ** 53 + 1, np.int64))


@pytest.mark.parametrize('src', R.SUPPORTED, ids=lambda d: d.name)
def test_cast_inputs_are_in_range(src):
  for dst in R.SUPPORTED:
    x = R.cast_inputs(src, dst)
    assert len(x) > 1000 or src.kind == 'f'
    if src.kind == 'f' and dst.kind in 'iu':
      assert len(x) > 500 and np.isfinite(x).all()
      ii = np.iinfo(dst)
      assert (np.trunc(x) >= ii.min).all() and (np.trunc(x.astype(np.longdouble)) <= ii.max).all()
    root = Cast(In(0, src), dst)
    with np.errstate(all='ignore'):
      got = np.asarray(eval_ir(root, {0: x}, x.shape))
      np.testing.assert_array_equal(R.bits(got), R.bits(x.astype(dst)))


def test_ulps():
  assert R.have_longdouble() == (np.finfo(np.longdouble).nmant >= 63)
  if not R.have_reference():
    pytest.skip('no long double wider than double and no mpmath')
  ld = np.longdouble
  one = np.float32(1)
  up = np.nextafter(one, np.float32(2))
  assert R.ulps(np.array([up]), np.array([ld(1)]), R.F32)[0] == 1
  assert R.ulps(np.array([np.nextafter(one, np.float32(0))]), np.array([ld(1)]), R.F32)[0] == 0.5
  sub = np.finfo(np.float32).smallest_subnormal
  assert R.ulps(np.array([sub * 3]), np.array([ld(sub) * 5]), R.F32)[0] == 2
  # an overflow counts from 2^128, and a result past it on both sides is no error
  assert R.ulps(np.array([np.float32(np.inf)]), np.array([ld(np.finfo(np.float32).max)]), R.F32)[0] == 1
  assert R.ulps(np.array([np.float32(np.inf)]), np.array([ld(1e300)]), R.F32)[0] == 0
  assert np.isinf(R.ulps(np.array([np.float32(np.nan)]), np.array([ld(1)]), R.F32)[0])
  want = R.expected_rounded('exp', (np.array([1.0]),))
  assert want.dtype == np.longdouble and abs(want[0] - ld('2.718281828459045235360287')) < 1e-18
  assert list(R.same_class(np.array([np.nan, -0.0, 0.0, -np.inf, 1.0]),
                           np.array([np.nan, -0.0, -0.0, -np.inf, 0.0], dtype=ld))) == [True, True, False, True, False]


@pytest.mark.parametrize('op', sorted(o for o in R.OPS if R.OPS[o]['cls'] != 'exact'))
def test_rounded_inputs_reach_domain_and_edges(op):
  """Rounded ops: most draws give finite, normal results, and the listed edges
  are present (NaN / inf / zero results exist too)."""
  if not R.have_reference():
    pytest.skip('no long double wider than double and no mpmath')
  for dt in R.FLOATS:
    args = R.inputs(op, dt)
    want = R.expected_rounded(op, args)
    num = R.numeric_mask(want)
    normal = num & (np.abs(want) >= np.finfo(dt).tiny) & (np.abs(want) <= np.finfo(dt).max)
    assert normal.sum() >= 1000, (op, dt, normal.sum())
    assert (~num).sum() >= 2, (op, dt)
