"""The generated map kernels on a real MI355X, lowering by lowering and path by
path: every case calls HipBackend.map (part c: HipBackend.reduce) on torch
tensors and compares every element with NumPy (tests/map_ref.py).

(a) values -- one test per (op, dtype) of map_ref.OPS: one dense launch over
    the pair's whole input vector, then the second operand as an Sc scalar for
    three scalars.  Exact-class ops must equal NumPy's result in the resolved
    dtype bit for bit (NaN payload free, signed zeros told apart).  Rounded
    ops must have the class and sign of a NaN / +-inf / +-0 long-double result
    and elsewhere hold two bounds: the project's relative contract RTOL where
    the result is a normal number (below the smallest normal the format's own
    spacing exceeds any relative bound, so only the ulp bound applies there),
    and the per-(op, dtype) ulp bound of ULP below.
(b) skeleton paths -- x0 * 3 + x1 - x2 on integer-valued, all-distinct data
    through views into NaN / sentinel-filled buffers; the launch's grid, its
    vector flag and the kernel's signature key are asserted before the values.
(c) the three reduce skeletons on the ops whose lowering was rewritten.
"""
import numpy as np
import pytest

import map_ref as R

pytestmark = pytest.mark.gpu

RTOL = {R.F32: 1e-5, R.F64: 1e-12}

# (op, result dtype) -> (kernel, NumPy, bound): the largest error in ulps of
# the generated kernel and of NumPy's own loop of that dtype, both against the
# long-double value on map_ref's inputs (all input dtypes and scalar forms of
# the pair), and the asserted bound: twice the kernel's figure rounded up to a
# whole ulp, at least 1 (room for a math-library update; the inputs are fixed,
# so a rerun reproduces the figure).  Every bound lies inside RTOL: 2^-23 per
# fp32 ulp and 2^-52 per fp64 ulp put RTOL at 83 and 4503 ulps.
ULP = {
    ('arccos', 'float32'): (1.248, 1.762, 3),
    ('arccos', 'float64'): (0.682, 0.782, 2),
    ('arcsin', 'float32'): (2.118, 2.274, 5),
    ('arcsin', 'float64'): (0.619, 0.749, 2),
    ('arctan', 'float32'): (1.669, 1.406, 4),
    ('arctan', 'float64'): (1.294, 0.500, 3),
    ('arctan2', 'float32'): (2.041, 2.835, 5),
    ('arctan2', 'float64'): (1.293, 0.737, 3),
    ('cbrt', 'float32'): (0.962, 1.757, 2),
    ('cbrt', 'float64'): (0.500, 0.530, 1),
    ('cos', 'float32'): (1.290, 1.251, 3),
    ('cos', 'float64'): (0.744, 0.507, 2),
    ('cosh', 'float32'): (0.546, 1.425, 2),
    ('cosh', 'float64'): (0.522, 0.750, 2),
    ('exp', 'float32'): (1.000, 2.113, 2),
    ('exp', 'float64'): (0.771, 0.616, 2),
    ('exp2', 'float32'): (0.672, 2.090, 2),
    ('exp2', 'float64'): (0.732, 0.666, 2),
    ('expm1', 'float32'): (0.927, 2.026, 2),
    ('expm1', 'float64'): (1.052, 0.507, 3),
    ('hypot', 'float32'): (1.318, 0.500, 3),
    ('hypot', 'float64'): (1.068, 0.531, 3),
    ('log', 'float32'): (1.848, 1.437, 4),
    ('log', 'float64'): (0.601, 0.542, 2),
    ('log10', 'float32'): (1.656, 1.998, 4),
    ('log10', 'float64'): (0.554, 0.500, 2),
    ('log1p', 'float32'): (0.528, 1.369, 2),
    ('log1p', 'float64'): (1.000, 0.567, 2),
    ('log2', 'float32'): (0.999, 1.303, 2),
    ('log2', 'float64'): (0.587, 0.500, 2),
    ('power', 'float32'): (1.103, 0.966, 3),
    ('power', 'float64'): (1.171, 0.667, 3),
    ('sin', 'float32'): (1.245, 1.245, 3),
    ('sin', 'float64'): (0.701, 0.513, 2),
    ('sinh', 'float32'): (0.865, 1.221, 2),
    ('sinh', 'float64'): (0.752, 0.714, 2),
    ('tan', 'float32'): (1.770, 2.383, 4),
    ('tan', 'float64'): (0.816, 0.540, 2),
    ('tanh', 'float32'): (1.270, 1.271, 3),
    ('tanh', 'float64'): (0.800, 1.053, 2),
}


def _be(gpu_ctx):
  from spartan_amd import backend
  be = backend.get()
  assert isinstance(be, backend.HipBackend)
  return be


def _dev(a):
  import torch
  return torch.from_numpy(np.array(a)).cuda()


def _map(be, root, ins, shape):
  import torch
  from spartan_amd import backend
  out = torch.empty(tuple(shape), dtype=backend.torch_dtype(root.dtype), device='cuda')
  be.map(root, ins, out)
  return out.cpu().numpy()


def _first_bad(bad, call):
  idx = np.flatnonzero(bad)[:5]
  return ['(%s)' % ', '.join(repr(c[i] if isinstance(c, np.ndarray) else c) for c in call) for i in idx], idx


def _check_exact(op, dt, call, got, label):
  want = R.expected_exact(op, call)
  assert got.dtype == want.dtype, (label, got.dtype, want.dtype)
  bad = R.bits(got) != R.bits(want)
  if bad.any():
    ops, idx = _first_bad(bad, call)
    raise AssertionError('%s: %d of %d differ from NumPy; first operands %s: kernel %r, NumPy %r'
                         % (label, bad.sum(), bad.size, ops, list(got[idx]), list(want[idx])))


def _check_rounded(op, root, call, got, label):
  if not R.have_reference():
    pytest.skip('no long double wider than double and no mpmath')
  rdt = root.dtype
  conv = [np.asarray(c).astype(t) for c, t in zip(call, root.in_dtypes)]
  want = R.expected_rounded(op, conv)
  yard = R.expected_exact(op, conv)  # NumPy's loop of the resolved dtype
  assert got.dtype == rdt == yard.dtype, (label, got.dtype)
  num = R.numeric_mask(want)
  u = R.ulps(got, want, rdt)
  un = R.ulps(yard, want, rdt)
  k_max, n_max = (float(np.max(x[num])) if num.any() else 0.0 for x in (u, un))
  print('MAPULP %s %s kernel=%.3f numpy=%.3f %s' % (op, rdt.name, k_max, n_max, label))
  bad = ~num & ~R.same_class(got, want)
  if bad.any():
    ops, idx = _first_bad(bad, call)
    raise AssertionError('%s: class or sign of a NaN / inf / zero result; operands %s: kernel %r, want %r'
                         % (label, ops, list(got[idx]), list(want[idx])))
  fi = np.finfo(rdt)
  with np.errstate(all='ignore'):
    aw = np.abs(want)
    normal = num & (aw >= fi.tiny) & (aw <= fi.max)
    rel = np.where(normal, np.abs(got.astype(np.longdouble) - want) / aw, 0)
  bad = ~(rel <= RTOL[rdt])
  if bad.any():
    ops, idx = _first_bad(bad, call)
    raise AssertionError('%s: relative error above %g; operands %s: kernel %r, want %r'
                         % (label, RTOL[rdt], ops, list(got[idx]), list(want[idx])))
  assert (op, rdt.name) in ULP, '%s: no ulp bound recorded; measured kernel %.3f, NumPy %.3f' % (label, k_max, n_max)
  bound = ULP[(op, rdt.name)][2]
  assert 1 <= bound and bound * 2.0 ** -fi.nmant <= RTOL[rdt]
  bad = num & ~(u <= bound)
  if bad.any():
    ops, idx = _first_bad(bad, call)
    raise AssertionError('%s: %.3f ulps, bound %d; operands %s: kernel %r, want %r'
                         % (label, k_max, bound, ops, list(got[idx]), list(want[idx])))


# ------------------------------------------------------------------ (a) values
@pytest.mark.parametrize('op,dt', R.pairs(), ids=['%s-%s' % (o, d.name) for o, d in R.pairs()])
def test_values(gpu_ctx, op, dt):
  from spartan_amd.codegen import In, Op, Sc
  be = _be(gpu_ctx)
  args = R.inputs(op, dt)
  dev = {i: _dev(a) for i, a in enumerate(args)}
  forms = [None] + (R.scalars(op, dt) if len(args) == 2 else [])
  for sc in forms:
    if sc is None:
      root, ins, call = Op(op, [In(i, dt) for i in range(len(args))]), dev, args
    else:
      root, ins, call = Op(op, [In(0, dt), Sc(0, sc)]), {0: dev[0]}, (args[0], sc)
    got = _map(be, root, ins, args[0].shape)
    label = '%s(%s%s)' % (op, dt.name, '' if sc is None else ', scalar %r' % (sc,))
    if R.op_class(op, dt) == 'exact':
      _check_exact(op, dt, call, got, label)
    else:
      _check_rounded(op, root, call, got, label)


_CASTS = [(s, d) for s in R.SUPPORTED for d in R.SUPPORTED if s != d]


@pytest.mark.parametrize('src,dst', _CASTS, ids=['%s-%s' % (s.name, d.name) for s, d in _CASTS])
def test_cast_values(gpu_ctx, src, dst):
  from spartan_amd.codegen import Cast, In
  x = R.cast_inputs(src, dst)
  got = _map(_be(gpu_ctx), Cast(In(0, src), dst), {0: _dev(x)}, x.shape)
  with np.errstate(all='ignore'):
    want = x.astype(dst)
  bad = R.bits(got) != R.bits(want)
  assert not bad.any(), 'cast %s -> %s: first operands %s' % (src, dst, _first_bad(bad, (x,))[0])


# ---------------------------------------------------------- (b) skeleton paths
SKEL_DTYPES = [R.F32, R.F64, R.I32, R.I64]
_ids = lambda d: d.name  # noqa: E731


def _fill(dt):
  return float('nan') if dt.kind == 'f' else (1 if dt.kind == 'b' else -77)


@pytest.fixture
def skel(gpu_ctx):
  """A HipBackend of this test's own, whose launches are recorded: the grid
  (launch_log), the vector flag of the argument block, and -- _sig_fns being
  empty before every call -- the signature key of the kernel it asked for."""
  from spartan_amd import backend
  be = backend.HipBackend()
  be.launch_log = []
  be.flags = []
  launch = be.launch

  def spy(fn, grid, args):
    be.flags.append(int(args.flags) & 1)
    return launch(fn, grid, args)
  be.launch = spy
  return be


def _buffer(n, dt):
  import torch
  from spartan_amd import backend
  return torch.full((n,), _fill(dt), dtype=backend.torch_dtype(dt), device='cuda')


def _view(vals, lead=16, pad=0, tail=16):
  """A device view holding ``vals`` (N-d host array) inside a NaN / sentinel
  buffer: ``lead`` elements before, ``pad`` after every innermost row, ``tail``
  at the end."""
  import torch
  vals = np.asarray(vals)
  shape = vals.shape if vals.ndim else (1,)
  pitch = shape[-1] + pad
  rows = int(np.prod(shape[:-1]))
  buf = _buffer(lead + rows * pitch + tail, vals.dtype)
  strides, acc = [1], pitch
  for s in reversed(shape[:-1]):
    strides.insert(0, acc)
    acc *= s
  v = torch.as_strided(buf, shape, tuple(strides), lead)
  v.copy_(torch.from_numpy(np.ascontiguousarray(vals).reshape(shape)))
  return v if vals.ndim else v[0]


def _expr(dts):
  """x0 * 3 + x1 - x2 (3 a weak Sc scalar)."""
  from spartan_amd.codegen import In, Op, Sc
  return Op('subtract', [Op('add', [Op('multiply', [In(0, dts[0]), Sc(0, 3)]), In(1, dts[1])]), In(2, dts[2])])


def _data(shapes, dt, full):
  """Integer-valued, all-distinct values per operand: broadcast to ``full`` the
  flat index i gives 3 i + (7 i + 5) - 2 i."""
  idx = np.arange(int(np.prod(full))).reshape(full)
  out = []
  for shape, (m, c) in zip(shapes, ((1, 0), (7, 5), (2, 0))):
    ps = (1,) * (len(full) - len(shape)) + tuple(shape)
    sl = tuple(slice(0, 1) if ps[d] == 1 else slice(None) for d in range(len(full)))
    out.append((idx[sl] * m + c).reshape(shape).astype(dt))
  return out


def _run_skel(be, root, ins, full, expect, per, mu=1):
  """Launch into a slice of a sentinel buffer; assert the path (signature key
  fields after the inputs: classes, ndim, V, dense, nt, mu; grid; vector
  flag), that nothing outside the slice was written, and return the result."""
  from spartan_amd import backend
  n = int(np.prod(full))
  odt = root.dtype
  obuf = _buffer(16 + n + 16, odt)
  out = obuf[16:16 + n].view(tuple(full))
  be._sig_fns.clear()
  del be.launch_log[:], be.flags[:]
  be.map(root, ins, out)
  (key,) = be._sig_fns
  assert key[0] == 'map' and key[1] == root.sig()
  assert key[3:] == expect, 'signature %r, this case was written for %r' % (key[3:], expect)
  assert be.launch_log == [max(1, -(-n // (256 * per * mu)))], (be.launch_log, n, per, mu)
  assert be.flags == [1 if per > 1 else 0]
  host = obuf.cpu().numpy()
  edge = np.concatenate([host[:16], host[16 + n:]])
  assert (np.isnan(edge) if odt.kind == 'f' else edge == _fill(odt)).all(), 'wrote outside the output slice'
  return host[16:16 + n].reshape(full)


def _want(vals):
  return vals[0] * 3 + vals[1] - vals[2]


def _dense_case(be, dt, n, lead=(16, 16, 16), nt=False, mu=1, vector=True):
  from spartan_amd import codegen
  V = codegen.vec_width([dt])
  vals = _data([(n,)] * 3, dt, (n,))
  ins = {k: _view(v, lead=lead[k]) for k, v in enumerate(vals)}
  per = V if vector else 1
  got = _run_skel(be, _expr([dt] * 3), ins, (n,), (('c', 'c', 'c'), 1, V, True, nt, mu if vector else 1), per,
                  mu if vector else 1)
  np.testing.assert_array_equal(got, _want(vals))


@pytest.mark.parametrize('dt', SKEL_DTYPES, ids=_ids)
def test_dense_vector_path(skel, dt):
  from spartan_amd import codegen
  V = codegen.vec_width([dt])
  for n in (V, 256 * V, 256 * V + V, 3 * 256 * V - V):
    _dense_case(skel, dt, n)


@pytest.mark.parametrize('dt', SKEL_DTYPES, ids=_ids)
def test_dense_scalar_fallback(skel, dt):
  from spartan_amd import codegen
  V = codegen.vec_width([dt])
  for n in sorted({1, V - 1, V + 1, 256 * V + 1}):
    _dense_case(skel, dt, n, vector=False)
  # a multiple of V, one input's base one element off 16-byte alignment
  _dense_case(skel, dt, 256 * V, lead=(16, 17, 16), vector=False)


@pytest.mark.parametrize('U', [2, 4])
@pytest.mark.parametrize('dt', SKEL_DTYPES, ids=_ids)
def test_dense_map_unroll(skel, monkeypatch, dt, U):
  """MAP_UNROLL U: the unrolled loop alone, with the tail loop, and the tail
  loop alone behind it."""
  from spartan_amd import backend, codegen
  monkeypatch.setattr(backend, 'MAP_UNROLL', U)
  V = codegen.vec_width([dt])
  for n in (256 * V * U - V, 256 * V * U, 256 * V * U + V, 2 * 256 * V * U + 256 * V):
    _dense_case(skel, dt, n, mu=U)
  _dense_case(skel, dt, 256 * V * U + 1, mu=U, vector=False)  # the scalar path is not unrolled


@pytest.mark.parametrize('dt', SKEL_DTYPES, ids=_ids)
def test_nontemporal_store_variant(skel, monkeypatch, dt):
  from spartan_amd import backend, codegen
  monkeypatch.setattr(backend, 'NT_STORE_BYTES', 0)
  V = codegen.vec_width([dt])
  for n in (256 * V + V, 3 * 256 * V - V):
    _dense_case(skel, dt, n, nt=True)
  monkeypatch.setattr(backend, 'MAP_UNROLL', 2)
  _dense_case(skel, dt, 256 * V * 2 + V, nt=True, mu=2)


# N-d operands: kind -> (shape of the operand for an (R, C) iteration space,
# class of its innermost dim, how the view is made)
def _nd_operand(kind, vals, V):
  import torch
  if kind == 'c':     # rows with an aligned pitch
    return _view(vals, pad=2 * V)
  if kind == 'c1':    # rows with a pitch that is no multiple of V
    return _view(vals, pad=2 * V + 1)
  if kind in ('row', 'col', '0d'):
    return _view(vals, pad=3)
  if kind == 'T':     # a transposed view: innermost stride is the pitch
    return _view(np.ascontiguousarray(vals.T), pad=5).t()
  assert kind == 's2'  # every second column of a wider buffer
  wide = np.full(vals.shape[:-1] + (2 * vals.shape[-1],), _fill(vals.dtype), dtype=vals.dtype)
  wide[..., ::2] = vals
  return _view(wide, pad=1)[..., ::2]


_ND_SHAPE = {'c': 'full', 'c1': 'full', 'T': 'full', 's2': 'full', 'row': 'row', 'col': 'col', '0d': '0d'}
_ND_CLASS = {'c': 'c', 'c1': 'c', 'row': 'c', 'col': 'b', '0d': 'b', 'T': 'g', 's2': 'g'}
ND_CASES = [  # operand kinds, vector path?, columns as a multiple of V plus a rest
    (('c', 'row', 'col'), True, 0), (('col', 'c', 'T'), True, 0), (('T', '0d', 'c'), True, 0),
    (('s2', 'c', 'row'), True, 0), (('0d', 'T', 's2'), True, 0), (('row', 's2', 'c'), True, 0),
    (('c1', 'row', 'col'), False, 0), (('col', 'T', 'c1'), False, 0),
    (('c', 'row', 'col'), False, 1), (('T', 'col', 'c'), False, 3),
]


@pytest.mark.parametrize('kinds,vector,rest', ND_CASES, ids=['%s%s' % ('-'.join(k), '+%d' % r if r else '')
                                                             for k, _, r in ND_CASES])
@pytest.mark.parametrize('dt', SKEL_DTYPES, ids=_ids)
def test_nd_classes(skel, dt, kinds, vector, rest):
  """(R, C) iteration space, every class in every slot: contiguous rows (aligned
  and unaligned pitch), a (1, C) row, an (R, 1) column, a 0-d tensor, a
  transposed view and a step-2 column slice."""
  from spartan_amd import codegen
  V = codegen.vec_width([dt])
  Rr, C = 37, 6 * V + rest
  shapes = [{'full': (Rr, C), 'row': (1, C), 'col': (Rr, 1), '0d': ()}[_ND_SHAPE[k]] for k in kinds]
  vals = _data(shapes, dt, (Rr, C))
  ins = {k: _nd_operand(kind, v, V) for k, (kind, v) in enumerate(zip(kinds, vals))}
  for k, kind in enumerate(kinds):
    assert tuple(ins[k].shape) == shapes[k]
  got = _run_skel(skel, _expr([dt] * 3), ins, (Rr, C), (tuple(_ND_CLASS[k] for k in kinds), 2, V, False, False, 1),
                  V if vector else 1)
  np.testing.assert_array_equal(got, _want(vals))


ND_SHAPES = [  # iteration space (last dim in units of V), operand shapes, dims left after coalescing
    ((5, 3), [(5, 3), (1, 3), (5, 3)], 2),
    ((3, 4, 2), [(3, 4, 2), (3, 1, 2), (1, 4, 2)], 3),
    ((3, 4, 2), [(3, 4, 2), (1, 1, 2), (3, 4, 2)], 2),       # dims 0 and 1 merge for every operand
    ((2, 3, 2, 2), [(2, 3, 2, 2), (2, 1, 2, 2), (1, 3, 1, 2)], 4),
    ((2, 2, 3, 2, 1), [(2, 2, 3, 2, 1), (2, 1, 3, 1, 1), (1, 2, 1, 2, 1)], 5),
]


@pytest.mark.parametrize('full,shapes,ndim', ND_SHAPES, ids=['%dd-%d' % (len(f), n) for f, _, n in ND_SHAPES])
@pytest.mark.parametrize('dt', [R.F32, R.I64], ids=_ids)
def test_nd_dims(skel, dt, full, shapes, ndim):
  """2 to 5 dims that the coalescer cannot merge (operands broadcast along
  alternating dims), and one shape it can."""
  from spartan_amd import codegen
  V = codegen.vec_width([dt])
  full = full[:-1] + (full[-1] * V,)
  shapes = [s[:-1] + (s[-1] * V,) for s in shapes]
  vals = _data(shapes, dt, full)
  ins = {k: _view(v, pad=V) for k, v in enumerate(vals)}
  got = _run_skel(skel, _expr([dt] * 3), ins, full, (('c', 'c', 'c'), ndim, V, False, False, 1), V)
  np.testing.assert_array_equal(got, _want(vals))


def test_nd_too_many_dims(skel):
  """More than MAX_DIM dims that do not coalesce: the documented refusal."""
  from spartan_amd import codegen
  full = (2,) * (codegen.MAX_DIM + 1)
  shapes = [full, tuple(2 if d % 2 == 0 else 1 for d in range(len(full))), full]
  vals = _data(shapes, R.F32, full)
  ins = {k: _dev(v) for k, v in enumerate(vals)}
  with pytest.raises(NotImplementedError, match='map over 9 non-coalescible dims'):
    _map(skel, _expr([R.F32] * 3), ins, full)
  assert skel.launch_log == []


def test_mixed_item_sizes(skel):
  from spartan_amd.codegen import In, Op
  # int8 + fp64: V = 2
  n = 256 * 2 + 2
  a, b = (np.arange(n) % 251 - 125).astype(np.int8), np.arange(n) * 0.5
  got = _run_skel(skel, Op('add', [In(0, R.I8), In(1, R.F64)]), {0: _view(a), 1: _view(b)}, (n,),
                  (('c', 'c'), 1, 2, True, False, 1), 2)
  np.testing.assert_array_equal(got, a + b)
  # bool xor int8 -> bool: V = 16
  n = 256 * 16 + 16
  a, b = np.arange(n) % 3 == 0, (np.arange(n) % 5 - 2).astype(np.int8)
  got = _run_skel(skel, Op('logical_xor', [In(0, R.B), In(1, R.I8)]), {0: _view(a), 1: _view(b)}, (n,),
                  (('c', 'c'), 1, 16, True, False, 1), 16)
  np.testing.assert_array_equal(got, np.logical_xor(a, b))
  # fp32 < fp32 -> bool out: V = 4, a 4-byte vector store
  n = 256 * 4 + 4
  a, b = np.arange(n, dtype=np.float32), (np.arange(n, dtype=np.float32)[::-1] * 2).copy()
  got = _run_skel(skel, Op('less', [In(0, R.F32), In(1, R.F32)]), {0: _view(a), 1: _view(b)}, (n,),
                  (('c', 'c'), 1, 4, True, False, 1), 4)
  np.testing.assert_array_equal(got, a < b)


def test_structure_max_inputs_and_scalars(skel):
  """MAX_IN array inputs, and every slot of both scalar tables (16 floats,
  16 ints)."""
  from spartan_amd import codegen
  from spartan_amd.codegen import In, Op, Sc
  n = 256 * 2 + 2
  xs = [(np.arange(n) * (k + 1) + k).astype(np.float64) for k in range(codegen.MAX_IN)]
  root, want = None, 0
  for k in range(codegen.MAX_IN):
    fs, isc = float(k) + 0.5, 3 - k
    term = Op('add', [Op('multiply', [In(k, R.F64), Sc(k, fs)]), Sc(k, isc)])
    root = term if root is None else Op('add', [root, term])
    want = xs[k] * fs + isc if k == 0 else want + (xs[k] * fs + isc)
  got = _run_skel(skel, root, {k: _view(x) for k, x in enumerate(xs)}, (n,),
                  (('c',) * 16, 1, 2, True, False, 1), 2)
  np.testing.assert_array_equal(got, want)


def test_structure_dag_consts_and_casts(skel):
  from spartan_amd.codegen import Cast, Const, In, Op
  n = 256 * 4 + 4
  x = (np.arange(n) - 500).astype(np.float32)
  leaf = In(0, R.F32)  # one object, used three times
  got = _run_skel(skel, Op('add', [Op('multiply', [leaf, leaf]), leaf]), {0: _view(x)}, (n,),
                  (('c',), 1, 4, True, False, 1), 4)
  np.testing.assert_array_equal(got, x * x + x)
  # Const leaves and a Cast chain fp64 -> fp32 -> int32 -> bool
  n = 256 * 2 + 2
  y = np.resize(np.array([0.0, 0.25, 1.5, -3.0, 1e-50, -0.75, 2.0 ** 31 - 200, -0.0, 123456.75]), n)
  chain = Cast(Cast(Cast(In(0, R.F64), R.F32), R.I32), R.B)
  root = Op('add', [Op('multiply', [Cast(chain, R.I64), Const(1000, R.I64)]), Const(41, R.I64)])
  got = _run_skel(skel, root, {0: _view(y)}, (n,), (('c',), 1, 2, True, False, 1), 2)
  np.testing.assert_array_equal(got, y.astype(np.float32).astype(np.int32).astype(bool).astype(np.int64) * 1000 + 41)


def test_empty_map_launches_nothing(skel):
  import torch
  x = torch.empty((0,), dtype=torch.float32, device='cuda')
  skel.map(_expr([R.F32] * 3), {0: x, 1: x, 2: x}, torch.empty((0,), dtype=torch.float32, device='cuda'))
  skel.map(_expr([R.F32] * 3), {0: x.view(0, 3), 1: x.view(0, 3), 2: x.view(0, 3)},
           torch.empty((0, 3), dtype=torch.float32, device='cuda'))
  assert skel.launch_log == [] and not skel._sig_fns


# ------------------------------------------------------- (c) reduce skeletons
def _grid_operands(dt, shape):
  a, b = R.decimal_grid(dt)
  n = int(np.prod(shape))
  idx = np.arange(n) * len(a) // n
  return a[idx].reshape(shape), b[idx].reshape(shape)


REDUCED = [('floor_divide', R.F32), ('floor_divide', R.F64), ('remainder', R.F32), ('remainder', R.F64),
           ('fmax', R.I32), ('fmin', R.I64), ('fmax', R.F32), ('fmin', R.F64),
           ('isinf', R.I32), ('isnan', R.I64), ('isfinite', R.I32)]


@pytest.mark.parametrize('shape', [(7, 300), (300, 5)], ids=['7x300', '300x5'])
@pytest.mark.parametrize('op,dt', REDUCED, ids=['%s-%s' % (o, d.name) for o, d in REDUCED])
def test_reduce_of_rewritten_ops(gpu_ctx, op, dt, shape):
  """sum and max of the op over every axis (rows / rowsp / cols skeletons share
  the Emitter).  max, integer sums and the sum of float floor_divide (small
  integers: exact in any order) must equal NumPy's; the other float sums
  (remainders, fmax / fmin of decimals) may differ by the rounding of another
  summation order, at most n eps sum|v| (the a-priori bound of recursive
  summation in any order)."""
  from spartan_amd.codegen import Cast, In, Op
  be = _be(gpu_ctx)
  a, b = _grid_operands(dt, shape)
  host = (a, b)[:R.OPS[op]['arity']]
  root = Op(op, [In(i, dt) for i in range(len(host))])
  if root.dtype == R.B:
    root = Cast(root, R.I32)
  with np.errstate(all='ignore'):
    vals = np.asarray(getattr(np, op)(*host)).astype(root.dtype)
  ins = {i: _dev(h) for i, h in enumerate(host)}
  for red in ('sum', 'max'):
    for axis in (None, 0, 1):
      oshape = () if axis is None else shape[:axis] + shape[axis + 1:]
      odt = np.dtype(np.int64) if (red == 'sum' and root.dtype.kind == 'i') else root.dtype
      got = be.reduce(root, red, ins, shape, axis, oshape, odt).cpu().numpy()
      want = getattr(np, red)(vals, axis=axis)
      label = '%s of %s(%s) %s axis %s' % (red, op, dt.name, shape, axis)
      if red == 'sum' and root.dtype.kind == 'f' and op != 'floor_divide':
        n = vals.size if axis is None else shape[axis]
        tol = n * np.finfo(dt).eps * np.sum(np.abs(vals.astype(np.float64)), axis=axis)
        assert (np.abs(got.astype(np.float64) - np.sum(vals.astype(np.longdouble), axis=axis)) <= tol).all(), label
      else:
        np.testing.assert_array_equal(got, np.asarray(want).astype(odt), err_msg=label)
