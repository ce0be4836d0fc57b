"""Paired sums on the CPU: the eligibility predicate over a table of views,
the paired kernel's source (what raises, what compiles for gfx950) and the
backend's bookkeeping of held row sums on stub tensors -- no device."""
import ctypes

import numpy as np
import pytest

from spartan_amd import backend, codegen
from spartan_amd.codegen import In, Op, RowDot, Sc

F32, F64, I32 = np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.int32)
NCU = 256


def _tree(dt, n=3):
  if n == 3:
    return Op('add', [Op('multiply', [In(0, dt), In(1, dt)]), Op('exp', [In(2, dt)])])
  return Op('add', [Op('multiply', [In(0, dt), Sc(0, 1.5)]), In(1, dt)])


def _plan(root, op, dts, view, res16=None):
  ins = [(k, dt) for k, dt in enumerate(dts)]
  plan = backend.plan_reduce(root, op, ins, res16 or [0] * len(dts), view, codegen.acc_dtype(op, root.dtype), None, NCU)
  return ins, plan


def _cols_view(R, I, n, O=1, pitch=None):
  pitch = pitch or I
  return (O, R, I, [(R * pitch, pitch, 1)] * n)


@pytest.fixture
def no_floor(monkeypatch):
  monkeypatch.setattr(backend, 'PAIR_MIN_BYTES', 0)


# ------------------------------------------------------------ eligibility
@pytest.mark.parametrize('dt,R,I', [(F32, 5, 256), (F32, 203, 512), (F32, 40, 64), (F64, 33, 128), (F64, 131, 384),
                                    (F32, 32768, 32768)])
def test_eligible_views(no_floor, dt, R, I):
  root = _tree(dt)
  view = _cols_view(R, I, 3)
  ins, plan = _plan(root, 'sum', [dt] * 3, view)
  assert plan.kind == 'cols' and backend.pair_eligible(root, 'sum', ins, view, plan)
  lpr, CT = 1 << plan.args.aux[2], plan.args.aux[3]
  assert I == CT * lpr * plan.V


def test_ineligible_views(no_floor):
  root = _tree(F32)
  # I no multiple of LPR * V (masked column tile)
  for I in (260, 96, 1028):
    view = _cols_view(64, I, 3)
    ins, plan = _plan(root, 'sum', [F32] * 3, view)
    assert plan.kind == 'cols' and not backend.pair_eligible(root, 'sum', ins, view, plan), I
  # an unaligned pointer residue: the scalar path
  view = _cols_view(64, 256, 3)
  ins, plan = _plan(root, 'sum', [F32] * 3, view, res16=[0, 4, 0])
  assert not plan.args.flags & 1 and not backend.pair_eligible(root, 'sum', ins, view, plan)
  # a row pitch that is no multiple of V: the scalar path too
  view = _cols_view(64, 256, 3, pitch=258)
  ins, plan = _plan(root, 'sum', [F32] * 3, view)
  assert not backend.pair_eligible(root, 'sum', ins, view, plan)
  # O > 1
  view = _cols_view(64, 256, 3, O=2)
  ins, plan = _plan(root, 'sum', [F32] * 3, view)
  assert plan.kind == 'cols' and not backend.pair_eligible(root, 'sum', ins, view, plan)
  # max and argmin
  view = _cols_view(64, 256, 3)
  for op in ('max', 'argmin'):
    ins, plan = _plan(root, op, [F32] * 3, view)
    assert not backend.pair_eligible(root, op, ins, view, plan), op
  # an integer tree
  iroot = Op('add', [In(0, I32), In(1, I32)])
  view = _cols_view(64, 256, 2)
  ins, plan = _plan(iroot, 'sum', [I32] * 2, view)
  assert plan.kind == 'cols' and not backend.pair_eligible(iroot, 'sum', ins, view, plan)
  # a row-dot tree (one 64-column tile)
  rd = Op('multiply', [In(0, F32), RowDot(In(0, F32), In(1, F32))])
  view = (1, 4096, 64, [(4096 * 64, 64, 1), (0, 0, 1)])
  ins, plan = _plan(rd, 'sum', [F32] * 2, view)
  assert plan.kind == 'cols' and not backend.pair_eligible(rd, 'sum', ins, view, plan)
  # a rows / rowsp view
  view = (64, 8192, 1, [(8192, 1, 0)] * 3)
  ins, plan = _plan(root, 'sum', [F32] * 3, view)
  assert plan.kind == 'rows' and not backend.pair_eligible(root, 'sum', ins, view, plan)


def test_byte_threshold_and_switch(monkeypatch):
  root = _tree(F32)
  assert backend.PAIR_MIN_BYTES == 64 << 20 and backend.PAIR_SUMS is True
  # 3 x 4 B x R x 1024 bytes read: 5461 rows stay one row short of 64 MiB
  for R, want in ((5461, False), (5462, True)):
    view = _cols_view(R, 1024, 3)
    ins, plan = _plan(root, 'sum', [F32] * 3, view)
    assert backend.pair_eligible(root, 'sum', ins, view, plan) is want, R
  # an input broadcast along the rows is read once
  view = (1, 5462, 1024, [(5462 * 1024, 1024, 1), (5462 * 1024, 1024, 1), (0, 0, 1)])
  ins, plan = _plan(root, 'sum', [F32] * 3, view)
  assert not backend.pair_eligible(root, 'sum', ins, view, plan)
  view = _cols_view(5462, 1024, 3)
  ins, plan = _plan(root, 'sum', [F32] * 3, view)
  monkeypatch.setattr(backend, 'PAIR_SUMS', False)
  assert not backend.pair_eligible(root, 'sum', ins, view, plan)


# ----------------------------------------------------------------- codegen
def _gen(root, dts, **kw):
  ins = [(k, dt) for k, dt in enumerate(dts)]
  a = dict(kind='cols', op='sum', vec=codegen.vec_width(list(dts)), lpr=64, full=True, interleave=False, pair=True)
  a.update(kw)
  return codegen.gen_reduce(root, ins, ['c'] * len(dts), a['kind'], a['op'], a['vec'], None, (), a['lpr'], a['full'],
                            a['interleave'], pair=a['pair'])


@pytest.mark.parametrize('kw', [dict(op='max'), dict(op='argmin'), dict(kind='rows'), dict(kind='rowsp'),
                                dict(interleave=True), dict(lpr=None), dict(full=False), dict(vec=1)])
def test_pair_kernel_refuses(kw):
  with pytest.raises(NotImplementedError):
    _gen(_tree(F32), [F32] * 3, **kw)


def test_pair_kernel_refuses_integer_and_rowdot():
  with pytest.raises(NotImplementedError):
    _gen(Op('add', [In(0, I32), In(1, I32)]), [I32] * 2)
  with pytest.raises(NotImplementedError):
    _gen(Op('multiply', [In(0, F32), RowDot(In(0, F32), In(1, F32))]), [F32] * 2)


@pytest.mark.parametrize('dt,lpr', [(F32, 16), (F32, 64), (F64, 16), (F64, 64)])
@pytest.mark.parametrize('n', [3, 2])
def test_pair_kernel_compiles(dt, lpr, n):
  """fp32 (V 4) and fp64 (V 2), 16 and 64 lanes per row; three inputs (one row
  per step) and two (the unrolled loop)."""
  assert codegen.vec_width([dt]) == (4 if dt == F32 else 2)
  src = _gen(_tree(dt, n), [dt] * n, lpr=lpr)
  assert 'a.out1' in src and src.count('KERN void spx_reduce') == 1
  assert ('r_1' in src) == (n == 2)
  backend.compile_code_object(src)


def test_unpaired_source_unchanged_by_the_keyword():
  ins = [(k, F32) for k in range(3)]
  a = codegen.gen_reduce(_tree(F32), ins, ['c'] * 3, 'cols', 'sum', 4)
  assert a == codegen.gen_reduce(_tree(F32), ins, ['c'] * 3, 'cols', 'sum', 4, pair=False)
  assert 'a.out1' not in a and 'asm volatile' not in a


# ------------------------------------------------------------- bookkeeping
class _Storage:
  def __init__(self, ptr, n):
    self._p, self._n = ptr, n

  def data_ptr(self):
    return self._p

  def nbytes(self):
    return self._n


class _T:
  """What the bookkeeping reads of a tensor."""
  def __init__(self, ptr, n, shape=(4, 4)):
    self._st = _Storage(ptr, n)
    self._version = 0
    self.shape = shape
    self.dtype = 'f32'

  def untyped_storage(self):
    return self._st


class _Lib:
  def __getattr__(self, name):
    return lambda *a: 0


@pytest.fixture
def be(monkeypatch):
  monkeypatch.setattr(backend, 'load_library', lambda: _Lib())
  monkeypatch.setattr(backend, 'current_stream', lambda: None)
  monkeypatch.setattr(backend, '_watch_eval_cache', lambda b: None)
  return backend.HipBackend()


def _hold(be, key, ts, root=None):
  rows = _T(0x900000, 64, shape=(4,))
  be._pair_hold(key, rows, root or _tree(F32, 2), {k: t for k, t in enumerate(ts)}, list(range(len(ts))))
  return rows


def _call(be, ptr):
  be._call('spx_fill', 0, 0, ctypes.c_void_p(ptr), timed=False)


def _launch(be, **kw):
  args = codegen.KArgs()
  for k, v in kw.items():
    if k == 'ptr':
      args.ptr[3] = v
    else:
      setattr(args, k, v)
  be.launch(ctypes.c_void_p(1), 1, args)


@pytest.mark.parametrize('via', ['call', 'ptr', 'out0', 'out1'])
@pytest.mark.parametrize('off,dropped', [(0, True), (4095, True), (100, True), (-1, False), (4096, False)])
def test_pointer_scan(be, via, off, dropped):
  x, y = _T(0x10000, 4096), _T(0x40000, 4096)
  _hold(be, 'k', [x, y])
  p = 0x40000 + off
  if via == 'call':
    _call(be, p)
  else:
    _launch(be, **{via: p})
  assert ('k' not in be._pair_memo) is dropped


def test_scan_not_entered_on_an_empty_table(be, monkeypatch):
  calls = []
  real = be._pair_scan
  monkeypatch.setattr(be, '_pair_scan', lambda ptrs: (calls.append(ptrs), real(ptrs)))
  _call(be, 0x40000)
  _launch(be, out0=0x40000)
  assert calls == []
  x = _T(0x10000, 4096)
  _hold(be, 'k', [x])
  _call(be, 0x80000)
  _launch(be, out0=0x80000)
  assert len(calls) == 2 and 'k' in be._pair_memo
  _call(be, 0x10000)
  assert len(calls) == 3 and not be._pair_memo
  _call(be, 0x10000)
  assert len(calls) == 3


def test_paired_launch_is_exempt_and_table_calls_clear(be, monkeypatch):
  x = _T(0x10000, 4096)
  _hold(be, 'k', [x])
  be._pair_own = True
  _call(be, 0x10000)
  _launch(be, ptr=0x10000)
  be._pair_own = False
  assert 'k' in be._pair_memo
  assert 'spx_sendrecv' in backend.PAIR_TABLE_CALLS
  be._call('spx_sendrecv', ctypes.c_void_p(0x80000), timed=False)
  assert not be._pair_memo


def _last(key, ts, root):
  import weakref
  return backend._PairLast(key, tuple(weakref.ref(t) for t in ts), backend._scalar_values(root))


def test_take_once_and_what_keeps_it(be, monkeypatch):
  monkeypatch.setattr(backend, 'torch_dtype', lambda dt: 'f32')
  root = _tree(F32, 2)
  x, y = _T(0x10000, 4096), _T(0x40000, 4096)
  ins, slots = {0: x, 1: y}, [0, 1]
  take = lambda last, key='k', r=root, i=ins, shape=(4,): be._pair_take(last, key, r, i, slots, shape, F32)
  rows = _hold(be, 'k', [x, y], root)
  assert 'k' not in be._pair_seen
  assert take(_last('k', [x, y], root)) is rows and not be._pair_memo and 'k' in be._pair_seen
  assert take(_last('k', [x, y], root)) is None  # handed over once
  # another key, another operand object, another scalar, a bumped version, another shape
  x2 = _T(0x10000, 4096)
  other = Op('add', [Op('multiply', [In(0, F32), Sc(0, 2.5)]), In(1, F32)])
  for last, kw in ((_last('j', [x, y], root), {}), (_last('k', [x2, y], root), {}),
                   (_last('k', [x, y], root), dict(i={0: x2, 1: y})), (_last('k', [x, y], other), {}),
                   (_last('k', [x, y], root), dict(r=other)), (_last('k', [x, y], root), dict(shape=(5,)))):
    _hold(be, 'k', [x, y], root)
    assert take(last, **kw) is None
  _hold(be, 'k', [x, y], root)
  y._version += 1
  assert take(_last('k', [x, y], root)) is None


def test_table_is_bounded_and_dead_operands_drop(be):
  keep = []
  for k in range(backend.PAIR_MEMO_MAX + 5):
    t = _T(0x10000 * (k + 1), 4096)
    keep.append(t)
    _hold(be, k, [t])
  assert len(be._pair_memo) == backend.PAIR_MEMO_MAX and 0 not in be._pair_memo
  last = backend.PAIR_MEMO_MAX + 4
  assert last in be._pair_memo
  keep.pop()
  del t
  assert last not in be._pair_memo
  be._reduce_plans.clear()
  assert not be._pair_memo and not be._pair_seen and be._pair_last is None


def test_eval_cache_clear_drops(monkeypatch):
  from spartan_amd.expr.base import eval_cache
  monkeypatch.setattr(backend, 'load_library', lambda: _Lib())
  b = backend.HipBackend()
  x = _T(0x10000, 4096)
  _hold(b, 'k', [x])
  eval_cache.set(-5, 'v')
  eval_cache.clear()
  assert not b._pair_memo and eval_cache.get(-5) is None
