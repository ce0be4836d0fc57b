"""backend.plan_reduce: the launch geometry of a fused map+reduce is pure
integer arithmetic on the (O, R, I) view, the pointer residues and the CU
count, so it is checked here without a device (256 CUs, the MI355X count).

The expected values were recorded from HipBackend.reduce before the planner
was split out of it (the kernel signature, grid, argument block and finalize
call of each case), not taken from plan_reduce; three carry their derivation."""
import numpy as np
import pytest

from spartan_amd import backend, codegen
from spartan_amd.codegen import In, Op, RowDot
from spartan_amd.layout import broadcast_strides, reduce_view

F32, F64, I64, B = (np.dtype(t) for t in (np.float32, np.float64, np.int64, np.bool_))


def plan(shapes, in_shape, axis, op='sum', dt=F32, root=None, res16=0, out_dtype=None, geom=None):
  """plan_reduce for contiguous operands of ``shapes`` (slot order) broadcast
  to ``in_shape``, every pointer at residue ``res16`` mod 16."""
  ins = [(s, dt) for s in range(len(shapes))]
  view = reduce_view(in_shape, [broadcast_strides(sh, in_shape) for sh in shapes], axis)
  root = root if root is not None else In(0, dt)
  if out_dtype is None:
    out_dtype = I64 if op in ('argmin', 'argmax') else codegen.acc_dtype(op, root.dtype)
  return backend.plan_reduce(root, op, ins, [res16] * len(shapes), view, out_dtype, geom, 256)


def rowdot_plan(K, dt=F32):
  x, y, w = In(0, dt), In(1, dt), In(2, dt)
  root = Op('multiply', [x, Op('subtract', [RowDot(x, w), y])])
  return plan([(7001, K), (7001, 1), (1, K)], (7001, K), 0, dt=dt, root=root)


def check(p, kind, V, flags, nblk, aux, direct, pdt, **gen):
  assert (p.kind, p.V, p.args.flags, p.nblk) == (kind, V, flags, nblk)
  assert list(p.args.aux) == list(aux) + [0] * (8 - len(aux))
  assert p.P == aux[0]  # aux[0..1] = (P, chunk) (rowsp: (1, R))
  assert (p.direct, p.pdt) == (direct, pdt)
  for name, want in gen.items():
    assert getattr(p, name) == want, name


def test_rows_flat():
  # (1, 2^20) fp32, all of it: V = 16 / 4 = 4; one segment, so P = min(2048 / 1,
  # ceil(2^20 / (256 lanes * 4 * 4 steps))) = 256 chunks of 2^20 / 256 = 4096;
  # grid = min(O * P, ROWS_GRID_PER_CU * CUs) = min(256, 2 * 256) = 256
  p = plan([(1, 1 << 20)], (1, 1 << 20), None)
  check(p, 'rows', 4, 1, 256, (256, 4096), False, F32, classes=('c',), U=None, n_out=1)


def test_rowsp_vector():
  # (1000, 100) fp32 over axis 1: R <= 64 * 4 * 16, so several segments per
  # wave; 100 / 4 = 25 vectors need 32 lanes (lpr_log 5): aux = (1, 100, 5);
  # 4 waves * (64 / 32) = 8 segments per block: grid = 1000 / 8 = 125
  p = plan([(1000, 100)], (1000, 100), 1)
  check(p, 'rowsp', 4, 1, 125, (1, 100, 5), True, F32)
  assert (p.args.dim[0], p.args.dim[1], p.args.dim[2]) == (1000, 100, 1)
  assert tuple(p.args.str[0][:3]) == (100, 1, 0)


@pytest.mark.parametrize('shape,res16', [((1000, 100), 4), ((1000, 101), 0)])
def test_rowsp_scalar_path(shape, res16):
  """A pointer one element off 16 bytes, or R no multiple of V: scalar loads,
  100 / 101 elements need 64 lanes, 4 segments per block."""
  p = plan([shape], shape, 1, res16=res16)
  check(p, 'rowsp', 4, 0, 250, (1, shape[1], 6), True, F32)


def test_rows_two_chunks_and_grid_cap():
  check(plan([(3, 5000)], (3, 5000), 1), 'rows', 4, 1, 6, (2, 2500), False, F32)
  # O >= 2048 segments: one chunk each, the grid capped at 2 per CU
  check(plan([(4096, 5000)], (4096, 5000), 1), 'rows', 4, 1, 512, (1, 5000), True, F32)


def test_cols():
  # one column tile: 2 lanes per row, 8 blocks per CU wanted, P limited by R
  check(plan([(5000, 8)], (5000, 8), 0), 'cols', 4, 1, 10, (10, 500, 1, 1), False, F32, U=4, rowinv=(), klpr=None,
        kint=False)
  # 4 column tiles of 64 lanes x 4: 2 blocks per CU -> P = 125
  check(plan([(5000, 1024)], (5000, 1024), 0), 'cols', 4, 1, 500, (125, 40, 6, 4), False, F32, U=4)
  # middle axis: O = 64 outer slices
  p = plan([(64, 5000, 8)], (64, 5000, 8), 1)
  check(p, 'cols', 4, 1, 640, (10, 500, 1, 1), False, F32, n_out=512)
  assert tuple(p.args.str[0][:3]) == (40000, 8, 1)
  # a (1, d) operand: row stride 0, loaded once per block
  p = plan([(5000, 8), (1, 8)], (5000, 8), 0, root=Op('multiply', [In(0, F32), In(1, F32)]))
  check(p, 'cols', 4, 1, 10, (10, 500, 1, 1), False, F32, classes=('c', 'c'), rowinv=(1,))
  # bool sum: int64 accumulator, V = 2
  check(plan([(5000, 8)], (5000, 8), 0, dt=B), 'cols', 2, 1, 20, (20, 250, 2, 1), False, I64)


def test_rowdot_full():
  # (7001, 64) fp32 x * (x.w - y) over axis 0: 64 / 4 = 16 lanes per row
  # (klpr 16), one column tile covered exactly (kfull), 4 * (64 / 16) = 16
  # rows per step; ROWDOT_BLOCKS_PER_CU = 1: P = min(256, ceil(7001 / (16 * 4)))
  # = 110 chunks of ceil(7001 / 110) = 64 rows; grid 110.  Interleaved fp32
  # sum: fp64 partials
  check(rowdot_plan(64), 'cols', 4, 1, 110, (110, 64, 4, 1), False, F64, classes=('c', 'b', 'c'), U=8, rowinv=(2,),
        klpr=16, kfull=True, kint=True)


def test_rowdot_masked_and_scalar(monkeypatch):
  check(rowdot_plan(48), 'cols', 4, 1, 110, (110, 64, 4, 1), False, F64, klpr=16, kfull=False, kint=True)
  check(rowdot_plan(5), 'cols', 4, 0, 55, (55, 128, 3, 1), False, F64, klpr=8, kfull=False, kint=True)
  check(rowdot_plan(33, F64), 'cols', 2, 0, 251, (251, 28, 6, 1), False, F64, klpr=64, kfull=False, kint=True)
  # the knobs are read at call time: contiguous chunks keep fp32 partials
  monkeypatch.setattr(backend, 'ROWDOT_INTERLEAVE', False)
  monkeypatch.setattr(backend, 'ROWDOT_BLOCKS_PER_CU', 16)
  check(rowdot_plan(64), 'cols', 4, 1, 110, (110, 64, 4, 1), False, F32, klpr=16, kfull=True, kint=False)


def test_arg_geometry():
  geom = {'decompose': True, 'tshape': (4, 50, 60), 'tul': (4, 0, 10), 'ashape': (16, 50, 100)}
  p = plan([(4, 50, 60)], (4, 50, 60), None, op='argmin', geom=geom)
  check(p, 'rows', 4, 1, 3, (3, 4000, 0, 0, 0, 1, 3), False, F32, arg=True)
  assert [tuple(a[:3]) for a in (p.args.tshape, p.args.tul, p.args.ashape)] == [(4, 50, 60), (4, 0, 10), (16, 50, 100)]
  p = plan([(2, 5, 6)], (2, 5, 6), None, op='argmin', geom=dict(geom, tshape=(2, 5, 6), ashape=(16, 5, 100)))
  check(p, 'rowsp', 4, 1, 1, (1, 60, 4, 0, 0, 1, 3), True, F32, arg=True)
  p = plan([(5000, 8)], (5000, 8), 0, op='argmax', geom={'offset': 7})
  check(p, 'cols', 4, 1, 10, (10, 500, 1, 1, 7), False, F32, arg=True)


def test_errors_and_empty():
  with pytest.raises(ValueError, match='zero-size reduction'):
    plan([(5, 0)], (5, 0), 1)
  x, y, w = In(0, F32), In(1, F32), In(2, F32)
  root = Op('multiply', [x, Op('subtract', [RowDot(x, w), y])])
  with pytest.raises(NotImplementedError, match='fused row dot needs each row in one lane group'):
    plan([(700, 512), (700, 1), (1, 512)], (700, 512), 0, root=root)
  p = plan([(0, 5)], (0, 5), 1)  # empty output: nothing to launch
  assert (p.nblk, p.n_out) == (0, 0)
