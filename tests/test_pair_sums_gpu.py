"""Paired sums on a real MI355X: the paired kernel (column sums + per-tile row
sums from one pass) at the smallest shapes at which each of its pieces can go
wrong, spx_reduce_finalize_pair called directly, and the backend's rules for
when an axis-1 sum is served from what the axis-0 pass left -- and when never.

Accuracy of the served axis-1 sum (random inputs): its largest relative error
against the fp64 NumPy sum may not exceed twice that of the unpaired row
kernel on the same inputs (an equally deep, differently shaped addition tree)
nor 1e-5.  PARENT_ROWS_ERR holds the unpaired kernel's figures, measured once
on an MI355X at the commit before the paired kernel existed.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
# dtype, shape, what it exercises
CASES = [(F32, (5, 256)),    # tail loop only, fewer rows than row groups
         (F32, (64, 256)),   # P = 4 row chunks
         (F32, (203, 512)),  # two column tiles, 13 row chunks, a short last chunk
         (F32, (40, 64)),    # LPR 16: four row groups per wave
         (F64, (33, 128)),   # V 2, LPR 64
         (F64, (131, 384))]  # three column tiles
TREES = ('exp', 'sc')        # x*y + exp(z);  x*1.5 + y (an Sc scalar, two inputs: the unrolled loop)
PARENT_ROWS_ERR = {
    ('f4', (5, 256), 'exp'): 4.5805949936485496e-08, ('f4', (5, 256), 'sc'): 6.228839437726748e-08,
    ('f4', (64, 256), 'exp'): 8.635304151274888e-08, ('f4', (64, 256), 'sc'): 1.0532810849192517e-07,
    ('f4', (203, 512), 'exp'): 8.590875791121013e-08, ('f4', (203, 512), 'sc'): 1.0470693229697604e-07,
    ('f4', (40, 64), 'exp'): 8.737785270680395e-08, ('f4', (40, 64), 'sc'): 9.817613404475964e-08,
    ('f8', (33, 128), 'exp'): 3.365757728480951e-16, ('f8', (33, 128), 'sc'): 1.8971311531579094e-16,
    ('f8', (131, 384), 'exp'): 4.1891904556077433e-16, ('f8', (131, 384), 'sc'): 2.382241504505374e-16,
}
_ids = ['%s-%dx%d' % (dt.name, s[0], s[1]) for dt, s in CASES]


def _tree(name, dt, scalar=1.5):
  from spartan_amd.codegen import In, Op, Sc
  if name == 'exp':
    return Op('add', [Op('multiply', [In(0, dt), In(1, dt)]), Op('exp', [In(2, dt)])]), 3
  if name == 'int':
    return Op('add', [Op('multiply', [In(0, dt), In(1, dt)]), In(2, dt)]), 3
  return Op('add', [Op('multiply', [In(0, dt), Sc(0, scalar)]), In(1, dt)]), 2


def _mapped(name, host, scalar=1.5):
  """The tree's values in fp64 from host operands."""
  h = [a.astype(np.float64) for a in host]
  if name == 'exp':
    return h[0] * h[1] + np.exp(h[2])
  if name == 'int':
    return h[0] * h[1] + h[2]
  return h[0] * scalar + h[1]


def _random(dt, shape, k):
  rs = np.random.RandomState(1000 + k)
  x = rs.rand(*shape).astype(dt)
  y = rs.rand(*shape).astype(dt)
  z = (rs.rand(*shape) * 2 - 1).astype(dt)
  return x, y, z


def _integers(dt, shape, k):
  """Small integers: every product, row sum and column sum is exact in fp32."""
  rs = np.random.RandomState(2000 + k)
  return tuple(rs.randint(-4, 5, size=shape).astype(dt) for _ in range(3))


def _dev(host):
  import torch
  return {i: torch.from_numpy(np.ascontiguousarray(h)).cuda() for i, h in enumerate(host)}


@pytest.fixture
def be(gpu_ctx):
  """A HipBackend of this test's own with the byte threshold off and its
  launches' names recorded; nothing seen, nothing held."""
  from spartan_amd import backend
  floor = backend.PAIR_MIN_BYTES
  backend.PAIR_MIN_BYTES = 0
  b = backend.HipBackend()
  b.kernel_events = []
  yield b
  backend.PAIR_MIN_BYTES = floor
  b._pair_reset()


def _names(be):
  """The launches logged since the last call."""
  n = [e[0] for e in be.kernel_events]
  del be.kernel_events[:]
  return n


def _sums(be, tree, dev, shape, dt, op='sum'):
  """The axis-0 then the axis-1 reduction: (host results, launch names of each)."""
  a0 = be.reduce(tree, op, dev, shape, 0, (shape[1],), dt)
  n0 = _names(be)
  a1 = be.reduce(tree, op, dev, shape, 1, (shape[0],), dt)
  n1 = _names(be)
  return (a0.cpu().numpy(), a1.cpu().numpy()), (n0, n1)


def _is(names, *kinds):
  return len(names) == len(kinds) and all(n.startswith('spx_reduce_' + k) for n, k in zip(names, kinds))


@pytest.mark.parametrize('tname', ['int', 'sc'])
@pytest.mark.parametrize('dt,shape', CASES, ids=_ids)
def test_integer_inputs_exact(be, dt, shape, tname):
  """Both results of the paired path equal the unpaired ones bit for bit, and NumPy's."""
  k = [s for _, s in CASES].index(shape)
  scalar = 3.0
  tree, n = _tree(tname, dt, scalar)
  host = _integers(dt, shape, k)[:n]
  dev = _dev(host)
  (u0, u1), (n0, n1) = _sums(be, tree, dev, shape, dt)
  assert _is(n0, 'cols') and _is(n1, 'rows')
  (p0, p1), (m0, m1) = _sums(be, tree, dev, shape, dt)
  assert _is(m0, 'pair') and m1 == []
  m = _mapped(tname, host, scalar)
  for got, unpaired, ax in ((p0, u0, 0), (p1, u1, 1)):
    assert got.dtype == dt
    np.testing.assert_array_equal(got, unpaired)
    np.testing.assert_array_equal(got, m.sum(axis=ax).astype(dt))


@pytest.mark.parametrize('tname', TREES)
@pytest.mark.parametrize('dt,shape', CASES, ids=_ids)
def test_random_inputs(be, dt, shape, tname):
  k = [s for _, s in CASES].index(shape)
  tree, n = _tree(tname, dt)
  host = _random(dt, shape, k)[:n]
  dev = _dev(host)
  (u0, u1), _ = _sums(be, tree, dev, shape, dt)
  (p0, p1), (m0, m1) = _sums(be, tree, dev, shape, dt)
  assert _is(m0, 'pair') and m1 == []
  np.testing.assert_array_equal(p0, u0)  # the column side is the unpaired kernel's, addition for addition
  want = _mapped(tname, host).sum(axis=1)
  rel = lambda got: float(np.max(np.abs(got.astype(np.float64) - want) / np.abs(want)))
  parent = PARENT_ROWS_ERR[(dt.str[1:], shape, tname)]
  print('%s %s %s: rows kernel %.4e (recorded %.4e), paired %.4e' % (dt.name, shape, tname, rel(u1), parent, rel(p1)))
  assert rel(p1) <= 2 * parent
  assert rel(p1) < 1e-5


def test_pattern_and_serving(be):
  dt, shape = F32, (64, 256)
  tree, n = _tree('exp', dt)
  host = _random(dt, shape, 1)
  dev = _dev(host)
  want = _mapped('exp', host).sum(axis=1)
  _, (n0, n1) = _sums(be, tree, dev, shape, dt)  # first occurrence: two launches, cols then rows
  assert _is(n0, 'cols') and _is(n1, 'rows')
  (_, p1), (m0, m1) = _sums(be, tree, dev, shape, dt)  # second: one launch, the axis-1 call logs nothing
  assert _is(m0, 'pair') and m1 == [] and not be._pair_memo
  np.testing.assert_allclose(p1, want, rtol=1e-5)
  again = be.reduce(tree, 'sum', dev, shape, 1, (shape[0],), dt)  # served once only
  assert _is(_names(be), 'rows')
  np.testing.assert_allclose(again.cpu().numpy(), want, rtol=1e-5)
  p1b = p1.copy()
  (_, p1c), (m0, m1) = _sums(be, tree, dev, shape, dt)  # deterministic
  assert _is(m0, 'pair') and m1 == []
  np.testing.assert_array_equal(p1c, p1b)


def _primed(be, tname='exp', scalar=1.5):
  """(64, 256) fp32 operands whose pair has been seen, after a paired axis-0 launch."""
  dt, shape = F32, (64, 256)
  tree, n = _tree(tname, dt, scalar)
  host = [h.copy() for h in _random(dt, shape, 1)[:n]]
  dev = _dev(host)
  _sums(be, tree, dev, shape, dt)
  be.reduce(tree, 'sum', dev, shape, 0, (shape[1],), dt)
  assert _is(_names(be), 'pair') and len(be._pair_memo) == 1
  return tree, host, dev, shape, dt


def _axis1(be, tree, dev, shape, dt, op='sum'):
  got = be.reduce(tree, op, dev, shape, 1, (shape[0],), dt)
  return got.cpu().numpy(), _names(be)


def test_never_served_after_a_torch_write(be):
  tree, host, dev, shape, dt = _primed(be)
  dev[0].add_(1.0)
  got, names = _axis1(be, tree, dev, shape, dt)
  assert _is(names, 'rows')
  np.testing.assert_allclose(got, _mapped('exp', [host[0] + 1, host[1], host[2]]).sum(axis=1), rtol=1e-5)


def test_never_served_after_a_fill(be):
  from spartan_amd import backend
  tree, host, dev, shape, dt = _primed(be)
  be.fill(dev[1], backend.FILL_CONST, 2.0, 0.0, 0, (0, 0), shape)
  assert not be._pair_memo
  got, names = _axis1(be, tree, dev, shape, dt)
  assert _is(names, 'rows')
  np.testing.assert_allclose(got, _mapped('exp', [host[0], np.full(shape, 2.0), host[2]]).sum(axis=1), rtol=1e-5)


def test_never_served_after_a_copy_region(be):
  import torch
  tree, host, dev, shape, dt = _primed(be)
  src = torch.full((8, 16), 3.0, dtype=torch.float32, device='cuda')
  be.copy_region(dev[2], (40, 100), src, (0, 0), (8, 16))
  assert not be._pair_memo
  z = host[2].copy()
  z[40:48, 100:116] = 3.0
  got, names = _axis1(be, tree, dev, shape, dt)
  assert _is(names, 'rows')
  np.testing.assert_allclose(got, _mapped('exp', [host[0], host[1], z]).sum(axis=1), rtol=1e-5)


def test_never_served_to_another_operand_object(be):
  tree, host, dev, shape, dt = _primed(be)
  other = dict(dev)
  other[0] = dev[0].clone()  # same layout, another object; then other values (its own _version only)
  other[0].mul_(2.0)
  got, names = _axis1(be, tree, other, shape, dt)
  assert _is(names, 'rows')
  np.testing.assert_allclose(got, _mapped('exp', [host[0] * 2, host[1], host[2]]).sum(axis=1), rtol=1e-5)


def test_never_served_with_another_scalar(be):
  tree, host, dev, shape, dt = _primed(be, 'sc', 1.5)
  tree2, _ = _tree('sc', dt, 2.5)
  assert tree2.sig() == tree.sig()
  got, names = _axis1(be, tree2, dev, shape, dt)
  assert _is(names, 'rows')
  np.testing.assert_allclose(got, _mapped('sc', host, 2.5).sum(axis=1), rtol=1e-5)


def test_never_served_to_a_max(be):
  tree, host, dev, shape, dt = _primed(be)
  got, names = _axis1(be, tree, dev, shape, dt, 'max')
  assert _is(names, 'rows')
  np.testing.assert_allclose(got, _mapped('exp', host).max(axis=1), rtol=1e-6)


def test_never_served_when_axis_1_comes_first(be):
  tree, host, dev, shape, dt = _primed(be)
  be._pair_memo.clear()
  want = _mapped('exp', host)
  got, names = _axis1(be, tree, dev, shape, dt)
  assert _is(names, 'rows')
  np.testing.assert_allclose(got, want.sum(axis=1), rtol=1e-5)
  a0 = be.reduce(tree, 'sum', dev, shape, 0, (shape[1],), dt)
  assert _is(_names(be), 'pair')
  np.testing.assert_allclose(a0.cpu().numpy(), want.sum(axis=0), rtol=1e-5)


def test_never_served_across_another_reduce(be):
  tree, host, dev, shape, dt = _primed(be)
  w = _dev([np.ones((16, 64), np.float32)])
  from spartan_amd.codegen import In
  s = be.reduce(In(0, F32), 'sum', w, (16, 64), 0, (64,), F32)
  _names(be)
  np.testing.assert_array_equal(s.cpu().numpy(), np.full(64, 16.0, np.float32))
  got, names = _axis1(be, tree, dev, shape, dt)
  assert _is(names, 'rows')
  np.testing.assert_allclose(got, _mapped('exp', host).sum(axis=1), rtol=1e-5)


def test_switched_off(be, monkeypatch):
  """PAIR_SUMS False: every launch and result is the unpaired path's."""
  from spartan_amd import backend
  dt, shape = F32, (203, 512)
  tree, n = _tree('exp', dt)
  dev = _dev(_random(dt, shape, 2))
  (u0, u1), _ = _sums(be, tree, dev, shape, dt)
  monkeypatch.setattr(backend, 'PAIR_SUMS', False)
  for _ in range(3):
    (g0, g1), (n0, n1) = _sums(be, tree, dev, shape, dt)
    assert _is(n0, 'cols') and _is(n1, 'rows') and not be._pair_memo and be._pair_last is None
    np.testing.assert_array_equal(g0, u0)
    np.testing.assert_array_equal(g1, u1)


@pytest.mark.parametrize('dt', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('P,CT', [(1, 1), (2, 3), (257, 128), (1, 128), (257, 1)])
def test_finalize_pair_direct(gpu_ctx, dt, P, CT):
  """Column partials: bit-equal to spx_reduce_finalize (P 257: its wide
  kernel); row partials: an fp64 fold in ct order, rounded once."""
  import torch
  from spartan_amd import backend
  be = backend.HipBackend()
  n, R = 37, 19
  rs = np.random.RandomState(P * 1000 + CT)
  cp = (rs.randn(P, n) * 100).astype(dt)
  rp = (rs.randn(CT, R) * 100).astype(dt)
  dcp, drp = torch.from_numpy(cp).cuda(), torch.from_numpy(rp).cuda()
  tdt = backend.torch_dtype(dt)
  cout = torch.full((n,), float('nan'), dtype=tdt, device='cuda')
  rout = torch.full((R,), float('nan'), dtype=tdt, device='cuda')
  ref = torch.full((n,), float('nan'), dtype=tdt, device='cuda')
  be._call('spx_reduce_finalize_pair', backend.spx_dtype(dt), backend._ptr(dcp), P, n, backend._ptr(cout),
           backend._ptr(drp), CT, R, backend._ptr(rout), timed=False)
  be.finalize('sum', dcp.reshape(-1), P, n, ref)
  np.testing.assert_array_equal(cout.cpu().numpy(), ref.cpu().numpy())
  acc = rp[0].astype(np.float64)
  for ct in range(1, CT):
    acc = acc + rp[ct].astype(np.float64)
  np.testing.assert_array_equal(rout.cpu().numpy(), acc.astype(dt))
