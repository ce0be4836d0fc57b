"""``spartan_amd.array.combine`` (no GPU): the combine-and-deliver route,
counted, over the CPU test double.

``PARENT`` holds, per case, the backend calls (merge, copy_region, finalize,
argcombine) and the collectives (all_reduce, reduce_scatter_rows,
all_gather_stack) that the operation made on the commit BEFORE the route moved
into ``array/combine.py`` (recorded there with this very test, printed and
pasted).  The one difference allowed since: where the engine's merged buffer
goes to an output that is one whole unwritten local tile, ``deliver`` adopts it
instead of copying it (``_adopts``: one ``copy_region`` fewer).
"""
import ast
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('merge', 'copy_region', 'finalize', 'argcombine', 'all_reduce', 'reduce_scatter_rows', 'all_gather_stack')
HINTS = [None, (10, 30), (40, 10), (20, 15)]
WORKERS = [1, 2, 4]
OPS = ['sum', 'sum0', 'sum1', 'min0', 'argmax', 'argmax0', 'argmax1', 'dot', 'dot_host', 'bincount']


@pytest.fixture
def counted(host_ctx, monkeypatch):
  """host_ctx whose test double counts the four backend calls, with counters
  on the three collectives: make(num_workers) -> the Counter."""
  import collections
  from spartan_amd import backend, comm
  from fake_backend import FakeBackend
  c = collections.Counter()

  def counting(fn, key):
    def f(*a, **kw):
      c[key] += 1
      return fn(*a, **kw)
    return f

  class Double(FakeBackend):
    pass
  for key in KEYS[:4]:
    setattr(Double, key, counting(getattr(FakeBackend, key), key))
  for key in KEYS[4:]:
    monkeypatch.setattr(comm, key, counting(getattr(comm, key), key))

  def make(num_workers=1):
    host_ctx(num_workers)
    backend.set_backend(Double())
    c.clear()
    return c
  return make


def _case(op, hint):
  """(build: () -> Expr, NumPy result) of one case of the table."""
  from spartan_amd import expr
  nx = np.arange(1200.).reshape(40, 30)
  ny = np.arange(600.).reshape(30, 20)
  if op == 'bincount':
    labels = np.arange(40) % 7
    v = expr.from_numpy(labels, tile_hint=hint and hint[:1]).force()
    return (lambda: expr.bincount(v)), np.bincount(labels)
  x = expr.from_numpy(nx, tile_hint=hint).force()
  if op == 'dot':
    y = expr.from_numpy(ny).force()
    return (lambda: expr.dot(x, y)), nx @ ny
  if op == 'dot_host':
    w = np.arange(30.).reshape(30, 1)
    return (lambda: expr.dot(x, w)), nx @ w
  name = op.rstrip('01')
  axis = int(op[-1]) if op[-1] in '01' else None
  return (lambda: getattr(expr, name)(x, axis)), getattr(nx, name)(axis)


def _run(counted, op, hint, W):
  c = counted(W)
  build, want = _case(op, hint)
  c.clear()
  out = build().force()
  got = tuple(c[k] for k in KEYS)
  np.testing.assert_array_equal(out.glom(), want)
  return got


# Recorded on the parent commit: (op, tile_hint, num_workers) -> KEYS counts.
PARENT = {
  ('sum', None, 1): (0, 0, 0, 0, 0, 0, 0),
  ('sum', None, 2): (2, 1, 0, 0, 0, 0, 0),
  ('sum', None, 4): (4, 1, 0, 0, 0, 0, 0),
  ('sum', (10, 30), 1): (4, 1, 0, 0, 0, 0, 0),
  ('sum', (10, 30), 2): (4, 1, 0, 0, 0, 0, 0),
  ('sum', (10, 30), 4): (4, 1, 0, 0, 0, 0, 0),
  ('sum', (40, 10), 1): (3, 1, 0, 0, 0, 0, 0),
  ('sum', (40, 10), 2): (3, 1, 0, 0, 0, 0, 0),
  ('sum', (40, 10), 4): (3, 1, 0, 0, 0, 0, 0),
  ('sum', (20, 15), 1): (4, 1, 0, 0, 0, 0, 0),
  ('sum', (20, 15), 2): (4, 1, 0, 0, 0, 0, 0),
  ('sum', (20, 15), 4): (4, 1, 0, 0, 0, 0, 0),
  ('sum0', None, 1): (0, 0, 0, 0, 0, 0, 0),
  ('sum0', None, 2): (2, 2, 0, 0, 0, 0, 0),
  ('sum0', None, 4): (4, 5, 0, 0, 0, 0, 0),
  ('sum0', (10, 30), 1): (4, 1, 0, 0, 0, 0, 0),
  ('sum0', (10, 30), 2): (4, 2, 0, 0, 0, 0, 0),
  ('sum0', (10, 30), 4): (4, 5, 0, 0, 0, 0, 0),
  ('sum0', (40, 10), 1): (3, 1, 0, 0, 0, 0, 0),
  ('sum0', (40, 10), 2): (3, 2, 0, 0, 0, 0, 0),
  ('sum0', (40, 10), 4): (3, 5, 0, 0, 0, 0, 0),
  ('sum0', (20, 15), 1): (4, 1, 0, 0, 0, 0, 0),
  ('sum0', (20, 15), 2): (4, 2, 0, 0, 0, 0, 0),
  ('sum0', (20, 15), 4): (4, 5, 0, 0, 0, 0, 0),
  ('sum1', None, 1): (0, 0, 0, 0, 0, 0, 0),
  ('sum1', None, 2): (0, 0, 0, 0, 0, 0, 0),
  ('sum1', None, 4): (0, 0, 0, 0, 0, 0, 0),
  ('sum1', (10, 30), 1): (4, 1, 0, 0, 0, 0, 0),
  ('sum1', (10, 30), 2): (4, 2, 0, 0, 0, 0, 0),
  ('sum1', (10, 30), 4): (0, 0, 0, 0, 0, 0, 0),
  ('sum1', (40, 10), 1): (3, 1, 0, 0, 0, 0, 0),
  ('sum1', (40, 10), 2): (3, 2, 0, 0, 0, 0, 0),
  ('sum1', (40, 10), 4): (3, 4, 0, 0, 0, 0, 0),
  ('sum1', (20, 15), 1): (4, 1, 0, 0, 0, 0, 0),
  ('sum1', (20, 15), 2): (4, 2, 0, 0, 0, 0, 0),
  ('sum1', (20, 15), 4): (4, 4, 0, 0, 0, 0, 0),
  ('min0', None, 1): (0, 0, 0, 0, 0, 0, 0),
  ('min0', None, 2): (2, 2, 0, 0, 0, 0, 0),
  ('min0', None, 4): (4, 5, 0, 0, 0, 0, 0),
  ('min0', (10, 30), 1): (4, 1, 0, 0, 0, 0, 0),
  ('min0', (10, 30), 2): (4, 2, 0, 0, 0, 0, 0),
  ('min0', (10, 30), 4): (4, 5, 0, 0, 0, 0, 0),
  ('min0', (40, 10), 1): (3, 1, 0, 0, 0, 0, 0),
  ('min0', (40, 10), 2): (3, 2, 0, 0, 0, 0, 0),
  ('min0', (40, 10), 4): (3, 5, 0, 0, 0, 0, 0),
  ('min0', (20, 15), 1): (4, 1, 0, 0, 0, 0, 0),
  ('min0', (20, 15), 2): (4, 2, 0, 0, 0, 0, 0),
  ('min0', (20, 15), 4): (4, 5, 0, 0, 0, 0, 0),
  ('argmax', None, 1): (0, 0, 0, 0, 0, 0, 0),
  ('argmax', None, 2): (0, 9, 0, 2, 0, 0, 0),
  ('argmax', None, 4): (0, 17, 0, 4, 0, 0, 0),
  ('argmax', (10, 30), 1): (0, 17, 0, 4, 0, 0, 0),
  ('argmax', (10, 30), 2): (0, 17, 0, 4, 0, 0, 0),
  ('argmax', (10, 30), 4): (0, 17, 0, 4, 0, 0, 0),
  ('argmax', (40, 10), 1): (0, 13, 0, 3, 0, 0, 0),
  ('argmax', (40, 10), 2): (0, 13, 0, 3, 0, 0, 0),
  ('argmax', (40, 10), 4): (0, 13, 0, 3, 0, 0, 0),
  ('argmax', (20, 15), 1): (0, 17, 0, 4, 0, 0, 0),
  ('argmax', (20, 15), 2): (0, 17, 0, 4, 0, 0, 0),
  ('argmax', (20, 15), 4): (0, 17, 0, 4, 0, 0, 0),
  ('argmax0', None, 1): (0, 0, 0, 0, 0, 0, 0),
  ('argmax0', None, 2): (0, 10, 0, 2, 0, 0, 0),
  ('argmax0', None, 4): (0, 21, 0, 4, 0, 0, 0),
  ('argmax0', (10, 30), 1): (0, 17, 0, 4, 0, 0, 0),
  ('argmax0', (10, 30), 2): (0, 18, 0, 4, 0, 0, 0),
  ('argmax0', (10, 30), 4): (0, 21, 0, 4, 0, 0, 0),
  ('argmax0', (40, 10), 1): (0, 13, 0, 3, 0, 0, 0),
  ('argmax0', (40, 10), 2): (0, 14, 0, 3, 0, 0, 0),
  ('argmax0', (40, 10), 4): (0, 17, 0, 3, 0, 0, 0),
  ('argmax0', (20, 15), 1): (0, 17, 0, 4, 0, 0, 0),
  ('argmax0', (20, 15), 2): (0, 18, 0, 4, 0, 0, 0),
  ('argmax0', (20, 15), 4): (0, 21, 0, 4, 0, 0, 0),
  ('argmax1', None, 1): (0, 0, 0, 0, 0, 0, 0),
  ('argmax1', None, 2): (0, 0, 0, 0, 0, 0, 0),
  ('argmax1', None, 4): (0, 0, 0, 0, 0, 0, 0),
  ('argmax1', (10, 30), 1): (0, 17, 0, 4, 0, 0, 0),
  ('argmax1', (10, 30), 2): (0, 18, 0, 4, 0, 0, 0),
  ('argmax1', (10, 30), 4): (0, 0, 0, 0, 0, 0, 0),
  ('argmax1', (40, 10), 1): (0, 13, 0, 3, 0, 0, 0),
  ('argmax1', (40, 10), 2): (0, 14, 0, 3, 0, 0, 0),
  ('argmax1', (40, 10), 4): (0, 16, 0, 3, 0, 0, 0),
  ('argmax1', (20, 15), 1): (0, 17, 0, 4, 0, 0, 0),
  ('argmax1', (20, 15), 2): (0, 18, 0, 4, 0, 0, 0),
  ('argmax1', (20, 15), 4): (0, 20, 0, 4, 0, 0, 0),
  ('dot', None, 1): (0, 0, 0, 0, 0, 0, 0),
  ('dot', None, 2): (0, 6, 0, 0, 0, 0, 0),
  ('dot', None, 4): (0, 24, 0, 0, 0, 0, 0),
  ('dot', (10, 30), 1): (0, 4, 0, 0, 0, 0, 0),
  ('dot', (10, 30), 2): (0, 10, 0, 0, 0, 0, 0),
  ('dot', (10, 30), 4): (0, 24, 0, 0, 0, 0, 0),
  ('dot', (40, 10), 1): (0, 3, 0, 0, 0, 0, 0),
  ('dot', (40, 10), 2): (0, 6, 0, 0, 0, 0, 0),
  ('dot', (40, 10), 4): (0, 11, 0, 0, 0, 0, 0),
  ('dot', (20, 15), 1): (0, 4, 0, 0, 0, 0, 0),
  ('dot', (20, 15), 2): (0, 6, 0, 0, 0, 0, 0),
  ('dot', (20, 15), 4): (0, 16, 0, 0, 0, 0, 0),
  ('dot_host', None, 1): (0, 0, 0, 0, 0, 0, 0),
  ('dot_host', None, 2): (0, 0, 0, 0, 0, 0, 0),
  ('dot_host', None, 4): (0, 0, 0, 0, 0, 0, 0),
  ('dot_host', (10, 30), 1): (4, 0, 0, 0, 0, 0, 0),
  ('dot_host', (10, 30), 2): (4, 2, 0, 0, 0, 0, 0),
  ('dot_host', (10, 30), 4): (0, 0, 0, 0, 0, 0, 0),
  ('dot_host', (40, 10), 1): (3, 0, 0, 0, 0, 0, 0),
  ('dot_host', (40, 10), 2): (3, 2, 0, 0, 0, 0, 0),
  ('dot_host', (40, 10), 4): (3, 4, 0, 0, 0, 0, 0),
  ('dot_host', (20, 15), 1): (4, 0, 0, 0, 0, 0, 0),
  ('dot_host', (20, 15), 2): (4, 2, 0, 0, 0, 0, 0),
  ('dot_host', (20, 15), 4): (4, 4, 0, 0, 0, 0, 0),
  ('bincount', None, 1): (0, 0, 0, 0, 1, 0, 0),
  ('bincount', None, 2): (4, 5, 0, 0, 1, 0, 0),
  ('bincount', None, 4): (8, 9, 0, 0, 1, 0, 0),
  ('bincount', (10, 30), 1): (8, 2, 0, 0, 1, 0, 0),
  ('bincount', (10, 30), 2): (8, 5, 0, 0, 1, 0, 0),
  ('bincount', (10, 30), 4): (8, 9, 0, 0, 1, 0, 0),
  ('bincount', (40, 10), 1): (0, 0, 0, 0, 1, 0, 0),
  ('bincount', (40, 10), 2): (0, 3, 0, 0, 1, 0, 0),
  ('bincount', (40, 10), 4): (0, 7, 0, 0, 1, 0, 0),
  ('bincount', (20, 15), 1): (4, 2, 0, 0, 1, 0, 0),
  ('bincount', (20, 15), 2): (4, 5, 0, 0, 1, 0, 0),
  ('bincount', (20, 15), 4): (4, 9, 0, 0, 1, 0, 0),
}


def _fewer(op, hint, W):
  """How many ``copy_region`` calls fewer than PARENT: one for every merged
  buffer of the engine's non-aligned path (it merged or arg-combined) that
  goes to an output of ONE tile, which now adopts it.  The outputs of one tile
  are the 0-d ones (axis None, at any number of workers; ``bincount`` makes
  two of them, the min and the max of its labels) and, with one worker, all.
  ``dot`` adopted before, and ``bincount``'s own delivery did."""
  merge, _, _, argcombine = PARENT[op, hint, W][:4]
  if op in ('dot', 'dot_host') or not (merge or argcombine):
    return 0
  if op == 'bincount':
    return 2
  return int(op in ('sum', 'argmax') or W == 1)


@pytest.mark.parametrize('W', WORKERS)
@pytest.mark.parametrize('hint', HINTS, ids=str)
@pytest.mark.parametrize('op', OPS)
def test_case_table(counted, op, hint, W):
  got = _run(counted, op, hint, W)
  print(op, hint, W, dict(zip(KEYS, got)))
  want = list(PARENT[op, hint, W])
  want[KEYS.index('copy_region')] -= _fewer(op, hint, W)
  assert got == tuple(want), dict(zip(KEYS, got))


# ------------------------------------------------------------ land, directly
def _target(shape, dtype, cuts, workers=None, overlap=None):
  """Unwritten 1-d / 2-d array cut along axis 0 at ``cuts`` (deferred tiles)."""
  from spartan_amd.array import blocks, extent as ext
  rest = tuple(shape[1:])
  exs = [ext.create((a,) + (0,) * len(rest), (b,) + rest, shape) for a, b in zip(cuts, cuts[1:])]
  return blocks.deferred(shape, dtype, {e: (workers[i] if workers else 0) for i, e in enumerate(exs)}), exs


def _counts(c):
  return c['merge'], c['copy_region']


def test_land_aligned_adopts(counted):
  import torch
  F64 = torch.float64
  from spartan_amd.array import combine
  c = counted(1)
  out, (e0, e1) = _target((4, 3), np.float64, [0, 2, 4])
  p0, p1 = torch.arange(6., dtype=F64).reshape(2, 3), torch.arange(6., 12., dtype=F64).reshape(2, 3)
  assert all(t._data is None for t in out.local.values())  # deferred: nothing allocated
  combine.land(out, [(e0, 0, p0), (e1, 0, p1)], 'sum')
  assert _counts(c) == (0, 0)
  assert out.local[e0]._data is p0 and out.local[e1]._data is p1
  assert out.local[e0].written == [e0]
  np.testing.assert_array_equal(out.glom(), np.arange(12.).reshape(4, 3))


def test_land_aligned_converts_another_dtype_once(counted):
  import torch
  F64 = torch.float64
  from spartan_amd.array import combine
  c = counted(1)
  out, (e0, e1) = _target((4, 3), np.float64, [0, 2, 4])
  p0, p1 = torch.arange(6, dtype=torch.int64).reshape(2, 3), torch.arange(6., 12., dtype=F64).reshape(2, 3)
  combine.land(out, [(e0, 0, p0), (e1, 0, p1)], 'sum')
  assert _counts(c) == (0, 1)
  assert out.local[e0]._data.dtype == torch.float64 and out.local[e1]._data is p1
  np.testing.assert_array_equal(out.glom(), np.arange(12.).reshape(4, 3))


def test_land_two_partials_on_one_destination_are_merged(counted):
  import torch
  F64 = torch.float64
  from spartan_amd.array import combine
  c = counted(1)
  out, (e0, e1) = _target((4, 3), np.float64, [0, 2, 4])
  ps = [torch.full((2, 3), float(v), dtype=F64) for v in (1, 2, 4)]
  parts = [(e0, 0, ps[0]), (e0, 0, ps[1]), (e1, 0, ps[2])]
  assert not combine.aligned(out, parts)
  combine.land(out, parts, 'sum')
  assert _counts(c) == (3, 2)  # three merges, one copy per tile
  np.testing.assert_array_equal(out.glom(), np.repeat([[3.], [4.]], 2, axis=0) * np.ones((4, 3)))


def test_land_overlapping_destinations_are_merged(counted):
  """Two destinations that overlap without being equal -- each of them a tile
  of an (ill-cut) output -- are merged, never adopted."""
  import torch
  F64 = torch.float64
  from spartan_amd.array import blocks, combine, extent as ext
  c = counted(1)
  ea, eb = ext.create((0,), (3,), (4,)), ext.create((2,), (4,), (4,))
  out = blocks.deferred((4,), np.float64, {ea: 0, eb: 0})
  parts = [(ea, 0, torch.ones(3, dtype=torch.float64)), (eb, 0, torch.full((2,), 2., dtype=torch.float64))]
  assert not combine.aligned(out, parts)
  assert combine.aligned(out, parts[:1]) and combine.aligned(out, parts[1:])
  combine.land(out, parts, 'sum')
  assert c['merge'] == 2
  np.testing.assert_array_equal(out.local[ea].data.numpy(), [1., 1., 3.])
  np.testing.assert_array_equal(out.local[eb].data.numpy(), [3., 2.])


def test_land_tile_of_another_rank_is_not_aligned(counted):
  """The verdict comes from the global metadata: a destination whose output
  tile belongs to the rank of another worker is not aligned."""
  import torch
  F64 = torch.float64
  from spartan_amd import runtime
  from spartan_amd.array import combine
  counted(2)
  ctx = runtime.get()
  out, (e0, e1) = _target((4, 3), np.float64, [0, 2, 4], workers=[0, 1])
  parts = [(e0, 0, torch.zeros(2, 3, dtype=torch.float64)), (e1, 1, torch.zeros(2, 3, dtype=torch.float64))]
  assert combine.aligned(out, parts)
  swapped = [(e0, 1, parts[0][2]), (e1, 0, parts[1][2])]
  assert combine.aligned(out, swapped)  # one rank owns both workers
  ctx.world_size = 2  # two ranks: worker k on rank k
  try:
    assert ctx.owner(0) != ctx.owner(1)
    assert combine.aligned(out, parts) and not combine.aligned(out, swapped)
    assert combine.aligned(out, [(e0, -1, None), (e1, -1, None)])  # a replicated input lands anywhere
  finally:
    ctx.world_size = 1


def test_land_aligned_never_allocates_a_deferred_tile(counted, monkeypatch):
  import torch
  F64 = torch.float64
  from spartan_amd.array import combine, tile
  counted(1)
  out, (e0,) = _target((4, 3), np.float32, [0, 4])
  t = out.local[e0]
  assert t._data is None
  monkeypatch.setattr(tile.Tile, 'data', property(lambda self: pytest.fail('the deferred tile was allocated'),
                                                  tile.Tile.data.fset))
  p = torch.ones(4, 3, dtype=torch.float64)  # another dtype: converted, still no allocation of the tile
  combine.land(out, [(e0, 0, p)], 'sum')
  assert t._data is not None and t._data.dtype == torch.float32
  q = torch.ones(4, 3, dtype=torch.float32)
  out2, (f0,) = _target((4, 3), np.float32, [0, 4])
  combine.land(out2, [(f0, 0, q)], 'sum')
  assert out2.local[f0]._data is q


# --------------------------------------------------------- deliver, directly
def test_deliver_whole_unwritten_tile_adopts(counted):
  import torch
  F64 = torch.float64
  from spartan_amd.array import combine
  c = counted(1)
  out, (e0,) = _target((4, 3), np.float64, [0, 4])
  full = torch.arange(12., dtype=F64).reshape(4, 3)
  combine.deliver(out, full)
  assert _counts(c) == (0, 0) and out.local[e0]._data is full and out.local[e0].written == [e0]


def test_deliver_written_tile_and_wrong_dtype_copy(counted):
  import torch
  F64 = torch.float64
  from spartan_amd.array import combine
  c = counted(1)
  full = torch.arange(12., dtype=F64).reshape(4, 3)
  out, (e0,) = _target((4, 3), np.float64, [0, 4])
  out.local[e0].data = torch.zeros(4, 3, dtype=torch.float64)
  out.local[e0].written = [e0]
  mine = out.local[e0]._data
  combine.deliver(out, full)
  assert _counts(c) == (0, 1) and out.local[e0]._data is mine
  np.testing.assert_array_equal(out.glom(), full.numpy())
  out, (e0,) = _target((4, 3), np.float32, [0, 4])
  combine.deliver(out, full)
  assert _counts(c) == (0, 2) and out.local[e0]._data.dtype == torch.float32
  np.testing.assert_array_equal(out.glom(), full.numpy().astype(np.float32))


def test_deliver_non_contiguous_ends_contiguous(counted):
  import torch
  F64 = torch.float64
  from spartan_amd.array import combine
  c = counted(1)
  full = torch.arange(12., dtype=F64).reshape(3, 4).t()
  assert not full.is_contiguous()
  out, (e0,) = _target((4, 3), np.float64, [0, 4])
  combine.deliver(out, full)
  assert _counts(c) == (0, 0) and out.local[e0]._data.is_contiguous()
  np.testing.assert_array_equal(out.glom(), np.arange(12.).reshape(3, 4).T)


def test_deliver_0d_and_four_tiles(counted):
  import torch
  F64 = torch.float64
  from spartan_amd.array import blocks, combine, extent as ext
  c = counted(1)
  e = ext.TileExtent((), (), ())
  out = blocks.deferred((), np.float64, {e: 0})
  v = torch.tensor(7., dtype=F64)
  combine.deliver(out, v)  # unwritten: adopted like any whole tile
  assert _counts(c) == (0, 0) and out.local[e]._data is v
  combine.deliver(out, torch.tensor(9., dtype=F64))  # written: the 0-d copy
  assert _counts(c) == (0, 1) and out.local[e]._data is v and float(v) == 9.0
  out, exs = _target((8, 3), np.float64, [0, 2, 4, 6, 8])
  full = torch.arange(24., dtype=F64).reshape(8, 3)
  combine.deliver(out, full)
  assert _counts(c) == (0, 5) and all(out.local[x].written == [x] for x in exs)
  np.testing.assert_array_equal(out.glom(), full.numpy())


# -------------------------------------------------------------------- static
def test_no_private_cross_layer_imports():
  pat = re.compile(r'from \.engine import _|from \.\.expr\.engine import _|examples\.kmeans import')
  pkg = os.path.join(ROOT, 'spartan_amd')
  hits = []
  for d, _, files in os.walk(pkg):
    for f in files:
      if f.endswith('.py'):
        with open(os.path.join(d, f)) as fh:
          hits += ['%s:%d' % (f, n) for n, line in enumerate(fh, 1) if pat.search(line)]
  assert hits == []
  with open(os.path.join(pkg, 'array', 'combine.py')) as fh:
    tree = ast.parse(fh.read())
  for node in ast.walk(tree):
    names = []
    if isinstance(node, ast.ImportFrom):
      names = [node.module or ''] + ['%s.%s' % (node.module or '', a.name) for a in node.names]
    elif isinstance(node, ast.Import):
      names = [a.name for a in node.names]
    for name in names:
      assert not set(name.split('.')) & {'expr', 'examples'}, name
