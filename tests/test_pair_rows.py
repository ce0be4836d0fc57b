"""The row side of the paired sums on the CPU: the paired kernel's source is
pinned (this work changed spx_reduce_finalize_pair's row half and left the
generated kernel alone: the names -- hashes of the source -- are those recorded
before it), the plans of the shapes that tests/test_pair_rows_gpu.py uses,
and a NumPy restatement of the documented order of a row sum's additions,
checked against itself here before the GPU test relies on it -- no device."""
import numpy as np
import pytest

from spartan_amd import backend, codegen
from spartan_amd.codegen import In, Op, Sc

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
NCU = 256
# named() of the paired kernel's source at LPR 64: the headline (x*y + exp(z),
# fp32, V 4, U 1) and the fp64 / two-input (unrolled) forms
PAIR_NAMES = {('exp', 'f4'): 'spx_reduce_pair_ab295997', ('exp', 'f8'): 'spx_reduce_pair_6343c4c1',
              ('sc', 'f4'): 'spx_reduce_pair_cba0e4c4', ('sc', 'f8'): 'spx_reduce_pair_ec7fe002'}


def _tree(name, dt):
  if name == 'exp':
    return Op('add', [Op('multiply', [In(0, dt), In(1, dt)]), Op('exp', [In(2, dt)])]), 3
  return Op('add', [Op('multiply', [In(0, dt), Sc(0, 1.5)]), In(1, dt)]), 2


@pytest.mark.parametrize('name,dts', sorted(PAIR_NAMES))
def test_paired_kernel_source_is_pinned(name, dts):
  dt = np.dtype(dts)
  root, n = _tree(name, dt)
  ins = [(k, dt) for k in range(n)]
  V = codegen.vec_width([dt])
  U = codegen.cols_unroll(ins, ('c',) * n, V)
  src = codegen.gen_reduce(root, ins, ('c',) * n, 'cols', 'sum', V, U, (), 64, True, False, pair=True)
  assert codegen.named(src, 'spx_reduce', 'pair')[1] == PAIR_NAMES[(name, dts)]


def test_unpaired_kernel_source_is_pinned():
  root, _ = _tree('exp', F32)
  src = codegen.gen_reduce(root, [(k, F32) for k in range(3)], ['c'] * 3, 'cols', 'sum', 4)
  assert codegen.named(src, 'spx_reduce', 'cols')[1] == 'spx_reduce_cols_8da20c40'


def test_the_shapes_of_the_gpu_tests():
  """What tests/test_pair_rows_gpu.py relies on: 64-lane row groups, (CT, P, rows of a chunk, of the last)."""
  def chunks(dt, R, I):
    root, n = _tree('exp', dt)
    view = (1, R, I, [(R * I, I, 1)] * n)
    p = backend.plan_reduce(root, 'sum', [(k, dt) for k in range(n)], [0] * n, view, dt, None, NCU)
    P, chunk, lpr, CT = p.args.aux[0], p.args.aux[1], 1 << p.args.aux[2], p.args.aux[3]
    assert lpr == 64 and CT > 1
    return CT, P, chunk, R - (P - 1) * chunk
  assert chunks(F32, 203, 512) == (2, 13, 16, 11)       # a short last chunk: waves with three rows and with two
  assert chunks(F32, 200, 768) == (3, 13, 16, 8)        # three column tiles
  assert chunks(F64, 131, 384) == (3, 9, 15, 11)
  assert chunks(F32, 66000, 512) == (2, 256, 258, 210)  # waves with 64 and 65 rows


# --------------------------------------------- the documented addition order
def documented_row_sums(vals, V, dt):
  """Row sums of ``vals`` (R, I) in the paired kernel's documented order, for
  LPR 64: per column tile of 64 * V columns the lane's V values folded in index
  order, the balanced binary tree over the 64 lanes (both in ``dt``), then the
  tiles folded in tile order in fp64 and rounded once to ``dt``."""
  R, I = vals.shape
  CT = I // (64 * V)
  assert I == CT * 64 * V and vals.dtype == dt
  v = vals.reshape(R, CT, 64, V)
  lane = v[..., 0]
  for j in range(1, V):
    lane = (lane + v[..., j]).astype(dt)
  while lane.shape[-1] > 1:
    lane = (lane[..., 0::2] + lane[..., 1::2]).astype(dt)
  part = lane[..., 0].astype(np.float64)  # (R, CT)
  acc = part[:, 0]
  for ct in range(1, CT):
    acc = acc + part[:, ct]
  return acc.astype(dt)


def test_documented_order_is_self_consistent():
  rs = np.random.RandomState(7)
  # small integers: every order gives the exact sum
  a = rs.randint(-4, 5, size=(9, 512)).astype(np.float32)
  np.testing.assert_array_equal(documented_row_sums(a, 4, F32), a.sum(axis=1, dtype=np.float64).astype(np.float32))
  # one tile of fp32: an explicit recursion over the 64 lanes gives the same bits
  b = rs.rand(5, 256).astype(np.float32)

  def tree(x):
    return x[0] if len(x) == 1 else np.float32(tree(x[:len(x) // 2]) + tree(x[len(x) // 2:]))
  want = [tree([np.float32(np.float32(np.float32(r[4 * j] + r[4 * j + 1]) + r[4 * j + 2]) + r[4 * j + 3])
                for j in range(64)]) for r in b]
  np.testing.assert_array_equal(documented_row_sums(b, 4, F32), np.array(want, np.float32))
  # the order matters at all: a sequential fold differs somewhere, and stays within rounding
  c = rs.rand(64, 512).astype(np.float32)
  seq = c[:, 0].copy()
  for j in range(1, 512):
    seq = (seq + c[:, j]).astype(np.float32)
  got = documented_row_sums(c, 4, F32)
  assert (got != seq).any()
  np.testing.assert_allclose(got, c.sum(axis=1, dtype=np.float64), rtol=1e-6)
  # fp64, V 2
  d = rs.rand(3, 384)
  np.testing.assert_allclose(documented_row_sums(d, 2, F64), d.sum(axis=1), rtol=1e-14)
