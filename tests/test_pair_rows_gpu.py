"""The row side of the paired sums on a real MI355X: spx_reduce_finalize_pair
called directly over the edges of its row half (blocks of 32 rows, passes of
128 column tiles: the fp64 fold in ct order, rounded once, bit for bit), and
the whole served axis-1 sum against a NumPy restatement of the documented
order of its additions and, on integer-valued inputs, against NumPy's sums."""
import numpy as np
import pytest

from test_pair_rows import documented_row_sums

pytestmark = pytest.mark.gpu

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
SHAPES = [(F32, (203, 512)), (F32, (200, 768)), (F64, (131, 384))]  # plans: tests/test_pair_rows.py
_ids = ['%s-%dx%d' % (dt.name, s[0], s[1]) for dt, s in SHAPES]


def _tree(name, dt, scalar=1.5):
  from spartan_amd.codegen import In, Op, Sc
  if name == 'int':
    return Op('add', [Op('multiply', [In(0, dt), In(1, dt)]), In(2, dt)]), 3
  return Op('add', [Op('multiply', [In(0, dt), Sc(0, scalar)]), In(1, dt)]), 2


def _dev(host):
  import torch
  return {i: torch.from_numpy(np.ascontiguousarray(h)).cuda() for i, h in enumerate(host)}


@pytest.fixture
def be(gpu_ctx):
  """A HipBackend of this test's own with the byte threshold off and its launches' names recorded."""
  from spartan_amd import backend
  floor = backend.PAIR_MIN_BYTES
  backend.PAIR_MIN_BYTES = 0
  b = backend.HipBackend()
  b.kernel_events = []
  yield b
  backend.PAIR_MIN_BYTES = floor
  b._pair_reset()


def _paired(be, tree, dev, shape, dt):
  """(axis-0 sums, served axis-1 sums) of the paired launch."""
  for k in range(2):  # the first pair is seen, the second runs paired and is served
    del be.kernel_events[:]
    a0 = be.reduce(tree, 'sum', dev, shape, 0, (shape[1],), dt)
    n0 = [e[0] for e in be.kernel_events]
    del be.kernel_events[:]
    a1 = be.reduce(tree, 'sum', dev, shape, 1, (shape[0],), dt)
    n1 = [e[0] for e in be.kernel_events]
  assert len(n0) == 1 and n0[0].startswith('spx_reduce_pair') and n1 == []
  return a0.cpu().numpy(), a1.cpu().numpy()


@pytest.mark.parametrize('dt,shape', SHAPES + [(F32, (66000, 512))], ids=_ids + ['float32-66000x512'])
def test_served_row_sums_in_the_documented_order(be, dt, shape):
  """x * 1.0 + y: with the scalar 1.0 a contracted and an uncontracted
  multiply-add give the same fl(x + y), so the documented order -- the lane's
  V values in index order, the balanced tree over the 64 lanes, the column
  tiles in order in fp64, rounded once -- holds to the bit.  (66000, 512):
  chunks of 258 rows, waves with 64 and 65 rows, 2063 blocks of the finalize."""
  rs = np.random.RandomState(3000 + shape[0])
  host = (rs.rand(*shape).astype(dt), rs.rand(*shape).astype(dt))
  tree, _ = _tree('sc', dt, 1.0)
  _, r = _paired(be, tree, _dev(host), shape, dt)
  np.testing.assert_array_equal(r, documented_row_sums((host[0] + host[1]).astype(dt), 4 if dt == F32 else 2, dt))


@pytest.mark.parametrize('dt,shape', SHAPES, ids=_ids)
def test_integer_inputs_exact(be, dt, shape):
  rs = np.random.RandomState(4000 + shape[0])
  host = tuple(rs.randint(-4, 5, size=shape).astype(dt) for _ in range(3))
  tree, _ = _tree('int', dt)
  c, r = _paired(be, tree, _dev(host), shape, dt)
  m = host[0].astype(np.float64) * host[1] + host[2]
  np.testing.assert_array_equal(c, m.sum(axis=0).astype(dt))
  np.testing.assert_array_equal(r, m.sum(axis=1).astype(dt))


def _finalize_pair(dt, P, n, CT, R, seed):
  """spx_reduce_finalize_pair on random partials: (columns, reference columns, rows, host row partials)."""
  import torch
  from spartan_amd import backend
  be = backend.HipBackend()
  rs = np.random.RandomState(seed)
  cp = (rs.randn(P, n) * 100).astype(dt)
  rp = (rs.randn(CT, R) * 100).astype(dt)
  dcp, drp = torch.from_numpy(cp).cuda(), torch.from_numpy(rp).cuda()
  tdt = backend.torch_dtype(dt)
  cout = torch.full((n,), float('nan'), dtype=tdt, device='cuda')
  rout = torch.full((R,), float('nan'), dtype=tdt, device='cuda')
  ref = torch.full((n,), float('nan'), dtype=tdt, device='cuda')
  be._call('spx_reduce_finalize_pair', backend.spx_dtype(dt), backend._ptr(dcp), P, n, backend._ptr(cout),
           backend._ptr(drp), CT, R, backend._ptr(rout), timed=False)
  if n:
    be.finalize('sum', dcp.reshape(-1), P, n, ref)
  return cout.cpu().numpy(), ref.cpu().numpy(), rout.cpu().numpy(), rp


def _ct_fold(rp, dt):
  acc = rp[0].astype(np.float64)
  for ct in range(1, rp.shape[0]):
    acc = acc + rp[ct].astype(np.float64)
  return acc.astype(dt)


@pytest.mark.parametrize('dt', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('CT', [1, 3, 128, 129, 300])
def test_finalize_pair_rows(gpu_ctx, dt, CT):
  """Rows: the fp64 fold in ct order, rounded once, bit for bit, over the
  edges of the 32-row blocks and the 128-ct passes; columns: spx_reduce_finalize's."""
  for R in (1, 31, 32, 33, 1000):
    cout, ref, rout, rp = _finalize_pair(dt, 3, 37, CT, R, CT * 10000 + R)
    np.testing.assert_array_equal(cout, ref)
    np.testing.assert_array_equal(rout, _ct_fold(rp, dt), err_msg='R = %d' % R)


@pytest.mark.parametrize('dt', [F32, F64], ids=['f32', 'f64'])
def test_finalize_pair_empty_halves(gpu_ctx, dt):
  cout, ref, rout, rp = _finalize_pair(dt, 2, 37, 3, 0, 1)  # R = 0 with n > 0
  np.testing.assert_array_equal(cout, ref)
  assert rout.shape == (0,)
  cout, ref, rout, rp = _finalize_pair(dt, 2, 0, 3, 33, 2)  # n = 0 with R > 0
  assert cout.shape == (0,)
  np.testing.assert_array_equal(rout, _ct_fold(rp, dt))
