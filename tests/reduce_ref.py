"""Host-only reference for the generated reduce kernels (codegen.gen_reduce's
three skeletons) and the two finalize kernels: the data, the cases, what each
case expects of the launch plan, and NumPy's result.  No GPU, no torch.

Data.  Every compared value is an integer, so a sum is exact in any order as
long as the sum of absolute values stays below 2^24 (fp32) / 2^53 (fp64):
``values`` gives, along every segment (the elements folded into one output),
non-zero integers of [-span, span] that are pairwise distinct within any
window of 2 * span consecutive elements -- a dropped element changes the sum,
and so does one element taken for another.  ``plant`` then puts extremes, ties
and NaNs where the kernels can go wrong (``edge_positions``), a different
scenario in every segment.

Cases.  ``CASES`` lists every path case of tests/test_reduce_gpu.py: shape,
axis, operand forms and the path it was written for (``expect``).  ``host_plan``
computes backend.plan_reduce for the same operand layouts without a device and
``check_plan`` asserts the path, so tests/test_reduce_ref.py checks every
expectation at 256 CUs and the GPU test checks the plan the backend really
used.  Literal P / grid values are never asserted (they depend on the CU
count; tests/test_reduce_plan.py pins the arithmetic).
"""
from collections import namedtuple

import numpy as np

F32, F64, I32, I64 = (np.dtype(t) for t in (np.float32, np.float64, np.int32, np.int64))
I8, U8, I16, B = (np.dtype(t) for t in (np.int8, np.uint8, np.int16, np.bool_))
MAIN = (F32, F64, I32, I64)
NARROW = (I8, U8, I16)
OPS = ('sum', 'min', 'max', 'argmin', 'argmax')
EMPTY = 0x7fffffffffffffff  # index of an empty (value, index) slot
SPAN = 500
BIG = 1 << 20  # planted float extreme (and the integer one of multi-operand cases): x0 = v - x1 + x2 stays exact in fp32


def exact_limit(dt):
  """Sums of absolute values below this are exact in ``dt`` in any order."""
  dt = np.dtype(dt)
  return {F32: 1 << 24, F64: 1 << 53}.get(dt, 1 << (8 * max(dt.itemsize, 8) - 1))


def span_for(dt):
  return 60 if np.dtype(dt) in NARROW else SPAN


# ------------------------------------------------------------------- data
def seg_values(nseg, R, span=SPAN, salt=0):
  """(nseg, R) int64: segment s, position r -> the k-th non-zero integer of
  [-span, span], k = (37 r + 101 s + salt) mod 2 span (37 is coprime to every
  2 span used, so 2 span consecutive r give 2 span distinct k)."""
  M = 2 * span
  assert np.gcd(37, M) == 1
  r = np.arange(R, dtype=np.int64)[None, :]
  s = np.arange(nseg, dtype=np.int64)[:, None]
  k = (37 * r + 101 * s + salt) % M
  return np.where(k < span, k + 1, span - 1 - k)


def seg_shape(shape, axis):
  """(nseg, R, outer shape, inner shape) of a reduction of ``shape`` over ``axis``."""
  shape = tuple(shape)
  if axis is None:
    return 1, int(np.prod(shape)), (), ()
  outer, inner = shape[:axis], shape[axis + 1:]
  return int(np.prod(outer + inner)), shape[axis], outer, inner


def from_segments(seg, shape, axis):
  """The array of ``shape`` whose segments along ``axis`` (in the order of the
  reduced result's flat index) are the rows of ``seg``."""
  nseg, R, outer, inner = seg_shape(shape, axis)
  assert seg.shape == (nseg, R)
  if axis is None:
    return np.ascontiguousarray(seg.reshape(shape))
  return np.ascontiguousarray(np.moveaxis(seg.reshape(outer + inner + (R,)), -1, axis))


def to_dtype(seg, dt):
  """Integer-valued ``seg`` in ``dt`` (unsigned: shifted to 1 .. 2 span)."""
  dt = np.dtype(dt)
  if dt.kind == 'u':
    seg = seg + int(np.abs(seg).max()) + 1
  out = seg.astype(dt)
  assert (out.astype(np.int64) == seg).all()
  return out


def values(shape, axis, dt, salt=0, span=None):
  span = span or span_for(dt)
  nseg, R, _, _ = seg_shape(shape, axis)
  return from_segments(to_dtype(seg_values(nseg, R, span, salt), dt), shape, axis)


def small_operand(shape, dt, salt):
  """A further operand of a multi-operand case: small non-zero integers,
  distinct within 2 * 97 consecutive elements of its own flat order."""
  n = int(np.prod(shape))
  k = (np.arange(n, dtype=np.int64) * 29 + salt) % 194
  return np.where(k < 97, k + 1, 96 - k).reshape(shape).astype(dt)


def edge_positions(kind, R, per, P, chunk, lanes, U):
  """{name: positions along a segment of length R} where a reduce kernel of
  this geometry can go wrong; two positions are an equal pair (a tie: the
  lower index must win).  per: elements per lane and step (V, scalar path 1);
  chunk: segment elements per block; lanes: per segment ('rowsp') / per row
  ('cols'); U: unrolled steps."""
  pos = {'first': [0], 'last': [R - 1]}
  if P > 1:
    pos['chunk_boundary'] = [chunk - 1, chunk]
  clen = min(chunk, R)
  if kind == 'cols':
    width = 4 * (64 // lanes)      # row groups of a block
    pair = [1, 2]
  else:
    width = (256 if kind == 'rows' else lanes) * per
    pair = [3 * per, 3 * per + 1] if per > 1 else [1, 2]
  if pair[1] < R:
    pos['one_vector'] = pair
  pos['last_lane'] = [min(clen, width) - 1]
  step = width * (U or 1)
  n_unrolled = max(0, -(-(clen - ((U or 1) - 1) * width) // step)) if (U or 1) > 1 else 0
  t = n_unrolled * step if kind != 'rowsp' else width
  pos['tail_loop'] = [t if t < clen else clen - 1]
  return {k: [p for p in v if 0 <= p < R] for k, v in pos.items()}


def scenarios(dt, positions):
  """[(what, positions)]: an extreme at the positions, for floats also a NaN
  there, and segments of all +inf / -inf / NaN."""
  out = [('ext', p) for p in positions.values()]
  if np.dtype(dt).kind == 'f':
    out += [('nan', p) for p in positions.values()] + [('pinf', None), ('ninf', None), ('allnan', None)]
  return out


def plant(seg, dt, side, scen, rnd=0, own=True):
  """``seg`` (nseg, R; integer-valued) in ``dt`` with scenario
  (s + rnd) mod len(scen) planted in segment s.  side 'lo': extremes for min /
  argmin, 'hi': for max / argmax.  Integer extremes are the type's own (every
  second scenario one inside it, so a read of the sentinel still shows);
  ``own`` False: +-BIG instead (multi-operand cases)."""
  dt = np.dtype(dt)
  out = to_dtype(seg, dt)
  nseg = out.shape[0]
  which = (np.arange(nseg) + rnd) % len(scen)
  for j, (what, pos) in enumerate(scen):
    segs = np.flatnonzero(which == j)
    if not len(segs):
      continue
    if what in ('pinf', 'ninf', 'allnan'):
      out[segs, :] = {'pinf': np.inf, 'ninf': -np.inf, 'allnan': np.nan}[what]
      continue
    if what == 'nan':
      v = np.nan
    elif dt.kind == 'f' or not own:
      v = -BIG if side == 'lo' else BIG
    else:
      ii = np.iinfo(dt)
      # (unsigned: the data starts at 1, so only 0 lies below it)
      v = (ii.min + (j % 2 if dt.kind == 'i' else 0)) if side == 'lo' else (ii.max - j % 2)
    for p in pos:
      out[segs, p] = v
  return out


def expected(vals, op, axis, odt):
  """NumPy's result of ``op`` over ``vals`` (arg ops: (values, indices))."""
  with np.errstate(all='ignore'):
    if op == 'sum':
      return np.asarray(vals.astype(np.int64).sum(axis=axis)).astype(odt)
    if op in ('min', 'max'):
      return np.asarray(getattr(np, op)(vals, axis=axis)).astype(odt)
    f = np.min if op == 'argmin' else np.max
    return np.asarray(f(vals, axis=axis)), np.asarray(getattr(np, op)(vals, axis=axis)).astype(np.int64)


def out_dtype(op, dt):
  """What the expr layer passes to backend.reduce: int64 for arg ops, else the value type."""
  return I64 if op in ('argmin', 'argmax') else np.dtype(dt)


def fill_value(dt, op):
  """The sentinel around a view: NaN; for integers the value that wins ``op``
  (a sum: one that visibly changes it)."""
  dt = np.dtype(dt)
  if dt.kind == 'f':
    return np.nan
  if dt.kind == 'b':
    return True
  ii = np.iinfo(dt)
  return {'sum': min(ii.max, 1000003), 'min': ii.min, 'argmin': ii.min, 'max': ii.max, 'argmax': ii.max}[op]


# --------------------------------------------------------- operand layouts
# form -> how an operand lies in its sentinel buffer: 'c' base and row pitch
# aligned to the vector; 'off' base one element off; 'pitch' row pitch no
# multiple of V; 'T' a transposed view (2-d: the innermost stride is the pitch);
# 'flat' contiguous (what a reduction over all dims of an N-d tile needs)
FORMS = ('c', 'off', 'pitch', 'T', 'flat')
Layout = namedtuple('Layout', 'lead strides total store_shape')


def layout(form, shape, V):
  """Where an operand of ``shape`` lies: elements before it, its strides, the
  buffer's length, and the shape it is stored in ('T': reversed)."""
  shape = tuple(shape) if len(shape) else (1,)
  store = shape[::-1] if form == 'T' else shape
  if form == 'T':
    assert len(shape) == 2
  pad = {'c': 2 * V, 'off': 2 * V, 'pitch': 2 * V + 1, 'T': 5, 'flat': 0}[form]
  lead = 17 if form == 'off' else 16
  pitch = store[-1] + pad
  strides, acc = [1], pitch
  for s in reversed(store[:-1]):
    strides.insert(0, acc)
    acc *= s
  rows = int(np.prod(store[:-1]))
  strides = tuple(strides[::-1]) if form == 'T' else tuple(strides)
  return Layout(lead, strides, lead + rows * pitch + 16, store)


# ------------------------------------------------------------------ cases
# operands: [(form, shape or None for the full shape)], slot order; expect:
# kind, vec (the vector flag), classes, U, rowinv and props (names of PROPS)
Case = namedtuple('Case', 'name dts shape axis operands expect ops vonly')


# cases whose shape exists for one vector width only.  The width follows the
# widest of input and accumulator: int32 sums (int64 accumulator) run with
# V = 2 and the other int32 ops with V = 4 (case_ops)
_W4, _W2 = (F32, I32), (F64, I64, I32)


def make_case(name, dts, shape, axis, kind, vec, props=(), operands=None, classes=None, U=None, rowinv=(), ops=OPS):
  operands = operands or [('c', None)]
  classes = classes or ('c',) * len(operands)
  vonly = 4 if dts is _W4 else 2 if dts is _W2 else None
  return Case(name, tuple(dts), shape, axis, tuple(operands),
              dict(kind=kind, vec=vec, classes=tuple(classes), U=U, rowinv=tuple(rowinv), props=tuple(props)), ops, vonly)


def _view_of(plan):
  return plan.args.dim[0], plan.args.dim[1], plan.args.dim[2]


PROPS = {
    'P>1': lambda p: p.P > 1,
    'P==1': lambda p: p.P == 1,
    'P==2': lambda p: p.P == 2,  # (two chunks per segment: a property of R and V, not of the CU count)
    'P>=32': lambda p: p.P >= 32,
    'CT>1': lambda p: p.args.aux[3] > 1,
    'CT==2': lambda p: p.args.aux[3] == 2,
    'CT==3': lambda p: p.args.aux[3] == 3,
    'CT==1': lambda p: p.args.aux[3] == 1,
    'O>1': lambda p: p.args.dim[0] > 1,
    'ragged': lambda p: p.args.dim[2] % ((1 << p.args.aux[2]) * (p.V if p.args.flags & 1 else 1)) != 0,
    'capped': lambda p: p.nblk < p.args.dim[0] * p.P,                  # rows: blocks walk several segments
    'rowsp_capped': lambda p: p.nblk == 4096 and p.nblk * 4 * (64 >> p.args.aux[2]) < p.args.dim[0],
    'last_block_short': lambda p: p.args.dim[0] % (4 * (64 >> p.args.aux[2])) != 0,  # rowsp: o >= O in the last block
    'trips>1': lambda p: p.args.dim[1] > (1 << p.args.aux[2]) * (p.V if p.args.flags & 1 else 1),
    'unrolled+tail': lambda p: _rows_unrolled_tail(p),
    'finalize': lambda p: not p.direct,
    'kint': lambda p: p.kint,
    'not kint': lambda p: not p.kint,
    'pdt f64': lambda p: p.pdt == F64,
    'folds middle sum': lambda p: _il_chunks(p) > 32 and _il_chunks(p) % 32 != 0,
}
for _u in (1, 2, 4):  # codegen.rows_unroll: steps of the rows loop per iteration (1, 2, 3 streamed operands: 4, 2, 1)
  PROPS['rows_unroll=%d' % _u] = (lambda u: lambda p: _rows_unroll(p) == u)(_u)
for _l in (1, 2, 4, 8, 16, 32, 64):
  PROPS['lanes=%d' % _l] = (lambda l: lambda p: (1 << p.args.aux[2]) == l)(_l)


def _rows_unroll(p):
  from spartan_amd import codegen
  return codegen.rows_unroll(None, p.classes)


def _rows_unrolled_tail(p):
  per = p.V if p.args.flags & 1 else 1
  U = 4  # single streamed operand
  clen = min(p.args.aux[1], p.args.dim[1])
  return clen > U * 256 * per and clen % (U * 256 * per) != 0


def _il_chunks(p):
  """Super-chunks (U steps of 4 * RPW rows) a block of an interleaved column sum walks."""
  rows = p.U * 4 * (64 >> p.args.aux[2])
  return -(-p.args.dim[1] // (rows * p.P))


def _by_v(f32, f64):
  """A shape that differs by vector width (V = 4: fp32 / int32, V = 2: fp64 / int64)."""
  return lambda V: f32 if V == 4 else f64


_ROWSP_LEN = [  # name, R as a function of V, vector path?, props
    ('R1', lambda V: 1, False, ('lanes=1',)), ('RV', lambda V: V, True, ('lanes=1',)),
    ('RV+1', lambda V: V + 1, False, ()), ('R2V', lambda V: 2 * V, True, ('lanes=2',)),
    ('R2V+1', lambda V: 2 * V + 1, False, ()), ('R3V', lambda V: 3 * V, True, ('lanes=4',)),
    ('R5V', lambda V: 5 * V, True, ('lanes=8',)), ('R9V', lambda V: 9 * V, True, ('lanes=16',)),
    ('R17V', lambda V: 17 * V, True, ('lanes=32',)), ('R33V', lambda V: 33 * V, True, ('lanes=64',)),
    ('R260', lambda V: 260, True, ('lanes=64', 'trips>1')),
    ('R1024V', lambda V: 1024 * V, True, ('lanes=64', 'trips>1')),
]
# (int32 sums stream 8-byte vectors of int32: cols_unroll gives them 4 and 2)
_NO_I32 = (F32, F64, I64)
_TWO = [('c', None), ('c', None)]
_THREE = [('c', None)] * 3

CASES = []
for _n, _R, _vec, _props in _ROWSP_LEN:
  CASES.append(make_case('rowsp-' + _n, MAIN, (lambda R: lambda V: (37, R(V)))(_R), 1, 'rowsp', _vec,
                  _props + ('last_block_short',), classes=('b',) if _n == 'R1' else None))
CASES += [
    make_case('rowsp-R2', _W4, (37, 2), 1, 'rowsp', False, ('lanes=2',)),
    make_case('rowsp-offset', MAIN, lambda V: (37, 9 * V), 1, 'rowsp', False, (), [('off', None)]),
    make_case('rowsp-pitch', MAIN, lambda V: (37, 9 * V), 1, 'rowsp', False, (), [('pitch', None)]),
    make_case('rowsp-gridcap', (F64,), (16400, 33), 1, 'rowsp', False, ('rowsp_capped', 'lanes=64')),
    make_case('rowsp-b-operand', MAIN, lambda V: (37, 9 * V), 1, 'rowsp', True, (), [('c', None), ('c', (37, 1))],
       classes=('c', 'b')),
    make_case('rowsp-transposed', MAIN, lambda V: (37, 9 * V), 1, 'rowsp', True, (), [('T', None)], classes=('g',)),

    make_case('rows-two-chunks', MAIN, _by_v((3, 4100), (3, 2052)), 1, 'rows', True, ('P==2', 'finalize', 'rows_unroll=4')),
    make_case('rows-two-chunks-offset', MAIN, _by_v((3, 4100), (3, 2052)), 1, 'rows', False, ('P>1', 'finalize'),
       [('off', None)]),
    make_case('rows-capped', MAIN, _by_v((2048, 4104), (2048, 2054)), 1, 'rows', True, ('P==1', 'capped', 'unrolled+tail')),
    make_case('rows-capped-P2', _W2, (600, 2052), 1, 'rows', True, ('P==2', 'capped')),
    make_case('rows-2-operands', MAIN, _by_v((3, 4100), (3, 2052)), 1, 'rows', True, ('P==2', 'rows_unroll=2'), _TWO),
    make_case('rows-3-operands', MAIN, _by_v((3, 4100), (3, 2052)), 1, 'rows', True, ('P==2', 'rows_unroll=1'), _THREE),
    make_case('rows-b-operand', MAIN, _by_v((3, 4100), (3, 2052)), 1, 'rows', True, ('P==2', 'rows_unroll=4'),
       [('c', None), ('c', (3, 1))], classes=('c', 'b')),
    make_case('rows-transposed', MAIN, (7, 5000), 1, 'rows', True, ('P>1',), [('T', None)], classes=('g',)),
    make_case('rows-flat', MAIN, (1, 8200), None, 'rows', True, ('P>1',)),

    make_case('cols-scalar-8-lanes', (F32, I32), (300, 5), 0, 'cols', False, ('P>1', 'lanes=8', 'CT==1'), U=4),
    make_case('cols-2-lanes', MAIN, lambda V: (520, 2 * V), 0, 'cols', True, ('lanes=2', 'CT==1'), U=4),
    make_case('cols-1-lane', MAIN, lambda V: (8200, V), 0, 'cols', True, ('lanes=1', 'CT==1'), U=4),
    make_case('cols-2-tiles', _W4, (300, 260), 0, 'cols', True, ('CT==2', 'ragged', 'P>1'), U=4),
    make_case('cols-3-tiles', _W2, (70, 300), 0, 'cols', True, ('CT==3', 'ragged', 'P>1'), U=4),
    make_case('cols-outer-partials', MAIN, (5, 70, 260), 1, 'cols', True, ('O>1', 'P>1', 'CT>1'), U=4),
    make_case('cols-P1-tiles', _W4, (256, 37, 260), 1, 'cols', True, ('P==1', 'CT==2', 'O>1'), U=4),
    make_case('cols-P1-narrow', _W4, (2048, 37, 8), 1, 'cols', True, ('P==1', 'CT==1', 'O>1'), U=4),
    make_case('cols-wide-finalize', _W2, (1000, 130), 0, 'cols', True, ('P>=32', 'CT==2'), U=4),
    make_case('cols-2-operands', _NO_I32, _by_v((300, 260), (70, 300)), 0, 'cols', True, ('P>1',), _TWO, U=2),
    make_case('cols-3-operands', _NO_I32, _by_v((300, 260), (70, 300)), 0, 'cols', True, ('P>1',), _THREE, U=1),
    make_case('cols-rowinv-b', MAIN, (300, 260), 0, 'cols', True, ('P>1',), [('c', None), ('c', (1, 260)), ('c', (300, 1))],
       classes=('c', 'c', 'b'), U=4, rowinv=(1,)),
    make_case('cols-transposed', MAIN, (300, 260), 0, 'cols', True, ('P>1',), [('T', None)], classes=('g',), U=4),
]
# the narrow integer types: one shape per skeleton and one P > 1 column shape
NARROW_CASES = [
    make_case('narrow-rowsp', NARROW, (37, 144), 1, 'rowsp', True, ('lanes=64',)),
    make_case('narrow-rows', NARROW, (3, 16400), 1, 'rows', True, ('P>1', 'finalize')),
    make_case('narrow-cols-P1', NARROW, (256, 37, 260), 1, 'cols', True, ('P==1', 'CT>1'), U=4),
    make_case('narrow-cols', NARROW, (300, 260), 0, 'cols', True, ('P>1', 'CT>1'), U=4),
]
# backend.COLS_INTERLEAVE = True (a knob: the case's ``knobs``)
IL_CASES = [
    make_case('il-f32-f64-partials', (F32,), (300, 260), 0, 'cols', True, ('kint', 'pdt f64', 'CT>1'), U=4, ops=('sum',)),
    make_case('il-f64-compensated', (F64,), (300, 130), 0, 'cols', True, ('kint', 'pdt f64', 'CT>1'), U=4, ops=('sum',)),
    make_case('il-max-not-interleaved', (F32,), (300, 260), 0, 'cols', True, ('not kint', 'CT>1'), U=4, ops=('max',)),
]
IL_BIG = make_case('il-middle-sum', (F32,), (256 * 530, 260), 0, 'cols', True, ('kint', 'pdt f64', 'folds middle sum'), U=4,
            ops=('sum',))
IL_BIG_SPAN = 60  # 135680 rows: sum|v| <= 60 * 135680 < 2^24


def case_v(dt, op):
  from spartan_amd import codegen
  return codegen.vec_width([dt, codegen.acc_dtype(op, dt)])


def case_ops(case, dt):
  """The case's ops that run on ``dt`` (all of them unless the case exists for one vector width only)."""
  return tuple(op for op in case.ops if case.vonly in (None, case_v(dt, op)))


def case_shape(case, dt, op):
  V = case_v(dt, op)
  return tuple(case.shape(V) if callable(case.shape) else case.shape)


def case_root(case, dt):
  """x0, x0 + x1 or x0 + x1 - x2 over the case's operands."""
  from spartan_amd.codegen import In, Op
  n = len(case.operands)
  root = In(0, dt)
  if n >= 2:
    root = Op('add', [root, In(1, dt)])
  if n == 3:
    root = Op('subtract', [root, In(2, dt)])
  return root


def case_operands(case, dt, vals):
  """Host operands (slot order) whose expression value is ``vals``: the
  further operands are small_operand's, x0 = vals - x1 + x2 (exact: |vals| <=
  BIG, NaN and inf carry over)."""
  shape = vals.shape
  rest = [small_operand(sh or shape, dt, 11 + 40 * k) for k, (_, sh) in enumerate(case.operands[1:])]
  x0 = vals
  with np.errstate(all='ignore'):
    if len(rest) >= 1:
      x0 = x0 - rest[0]
    if len(rest) == 2:
      x0 = x0 + rest[1]
  return [np.ascontiguousarray(np.broadcast_to(x0, shape)).astype(dt)] + rest


def host_plan(case, dt, op, ncu=256, V=None, geom=None, in_dts=None):
  """backend.plan_reduce for the case's operand layouts, no device: buffers
  are taken as 16-byte aligned (torch's allocations are)."""
  from spartan_amd import backend, codegen
  from spartan_amd.layout import broadcast_strides, reduce_view
  shape = case_shape(case, dt, op)
  root = case_root(case, dt)
  in_dts = in_dts or [dt] * len(case.operands)
  V = V or codegen.vec_width(list(in_dts) + [codegen.acc_dtype(op, root.dtype)])
  strides, res16 = [], []
  for (form, sh), idt in zip(case.operands, in_dts):
    sh = tuple(sh or shape)
    lay = layout(form, sh, V)
    strides.append(broadcast_strides(sh, shape, lay.strides))
    res16.append(lay.lead * np.dtype(idt).itemsize % 16)
  view = reduce_view(shape, strides, case.axis)
  assert view is not None, 'case %s: the operands do not collapse to (O, R, I)' % case.name
  ins = [(k, np.dtype(t)) for k, t in enumerate(in_dts)]
  return backend.plan_reduce(root, op, ins, res16, view, out_dtype(op, root.dtype), geom, ncu)


def check_plan(case, plan, op=None):
  """AssertionError naming the path the case was written for unless ``plan`` is on it."""
  e = case.expect
  got = dict(kind=plan.kind, vec=bool(plan.args.flags & 1), classes=tuple(plan.classes), rowinv=tuple(plan.rowinv))
  want = {k: e[k] for k in got}
  if e['U'] is not None:
    got['U'], want['U'] = plan.U, e['U']
  assert got == want, 'case %s: plan %r, this case was written for %r' % (case.name, got, want)
  for name in e['props']:
    assert PROPS[name](plan), ('case %s: plan (P %d, grid %d, aux %s) is not "%s", which this case was written for'
                               % (case.name, plan.P, plan.nblk, list(plan.args.aux), name))


def geometry(plan):
  """edge_positions' arguments of a plan."""
  per = plan.V if plan.args.flags & 1 else 1
  R = plan.args.dim[1]
  if plan.kind == 'rowsp':
    return dict(kind='rowsp', R=R, per=per, P=1, chunk=R, lanes=1 << plan.args.aux[2], U=1)
  if plan.kind == 'rows':
    from spartan_amd import codegen
    return dict(kind='rows', R=R, per=per, P=plan.P, chunk=plan.args.aux[1], lanes=256,
                U=codegen.rows_unroll(None, plan.classes))
  return dict(kind='cols', R=R, per=per, P=plan.P, chunk=plan.args.aux[1], lanes=1 << plan.args.aux[2], U=plan.U)


# -------------------------------------------------- finalize / arg-combine
def fold(op, parts):
  """Plain fold over axis 0 of (P, n) partials in p order (np.minimum /
  np.maximum: NaN propagates)."""
  f = {'sum': np.add, 'min': np.minimum, 'max': np.maximum}[op]
  acc = parts[0].copy()
  with np.errstate(all='ignore'):
    for p in range(1, parts.shape[0]):
      acc = f(acc, parts[p])
  return acc


def arg_fold(op, vals, idx):
  """(values, indices) of the best of (P, n) (value, index) partials: empty
  slots never win, the first NaN (lowest index) wins, equal values go to the
  lowest index."""
  bv, bi = vals[0].copy(), idx[0].copy()
  isf = vals.dtype.kind == 'f'
  for p in range(1, vals.shape[0]):
    v, vi = vals[p], idx[p]
    better = np.where(v == bv, vi < bi, (v < bv) if op == 'argmin' else (v > bv))
    if isf:
      vn, bn = np.isnan(v), np.isnan(bv)
      better = np.where(vn | bn, vn & (~bn | (vi < bi)), better)
    take = (vi != EMPTY) & ((bi == EMPTY) | better)
    bv, bi = np.where(take, v, bv), np.where(take, vi, bi)
  return bv, bi
