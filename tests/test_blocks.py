"""``spartan_amd.array.blocks`` (no GPU): the exchanges of the three block
routes, counted, over the CPU test double.

A ``gather_regions`` carries one ``comm.exchange`` of its own; the counters
keep that one apart (``inner``) from the exchanges issued outside a gather
(``exchanges``: the ``scatter_updates`` batch).  The expected counts are those
the operations gave before the routes moved into ``blocks``: routes 1 and 2
issue no gather and no exchange, route 3 one gather and one scatter.
"""
import numpy as np
import pytest

SHAPE = (6, 5)
# one tile; row strips; column strips; a 2 x 2 grid -- and the route of an operation along axis 1
LAYOUTS = [((6, 5), 2), ((2, 5), 2), ((6, 2), 3), ((3, 3), 3)]


class Counts:
  def __init__(self):
    self.gathers, self.exchanges, self.inner = [], 0, 0

  def reset(self):
    self.__init__()

  def routes(self):
    return len(self.gathers), self.exchanges


@pytest.fixture
def counts(monkeypatch):
  """Counts ``distarray.gather_regions`` (the number of requests of each call)
  and ``comm.exchange`` (inside a gather / outside)."""
  from spartan_amd import comm
  from spartan_amd.array import distarray
  c = Counts()
  gather, exchange = distarray.gather_regions, comm.exchange
  depth = []

  def counted_gather(array, requests):
    c.gathers.append(len(requests))
    depth.append(1)
    try:
      return gather(array, requests)
    finally:
      depth.pop()

  def counted_exchange(sends, recvs):
    if depth:
      c.inner += 1
    else:
      c.exchanges += 1
    return exchange(sends, recvs)
  monkeypatch.setattr(distarray, 'gather_regions', counted_gather)
  monkeypatch.setattr(comm, 'exchange', counted_exchange)
  return c


@pytest.fixture
def blocks_ctx(host_ctx):
  """host_ctx with a test double that sorts, selects and pools."""
  from spartan_amd import backend
  from stencil_ref import StencilFakeBackend
  from topk_ref import TopkFakeBackend

  class Double(TopkFakeBackend, StencilFakeBackend):
    pass

  def make(num_workers=1):
    host_ctx(num_workers)
    backend.set_backend(Double())
  return make


def _data(shape=SHAPE):
  return np.random.RandomState(5).permutation(int(np.prod(shape))).reshape(shape).astype(np.float32)


def _tiled(a, hint):
  from spartan_amd import expr
  return expr.from_numpy(a, tile_hint=hint).force()


def _replicated(a):
  import torch
  from spartan_amd.array import distarray
  return distarray.ReplicatedArray(torch.as_tensor(a.copy()))


@pytest.mark.parametrize('W', [1, 3])
def test_map_blocks_routes(blocks_ctx, counts, W):
  blocks_ctx(W)
  from spartan_amd.array import blocks, distarray
  a = _data()
  plus_one = lambda t, shape: t + 1
  for hint, route in LAYOUTS:
    arr = _tiled(a, hint)
    assert blocks.spans(arr, (1,)) == (route == 2), hint
    counts.reset()
    out = blocks.map_blocks(arr, (1,), 0, plus_one)
    assert counts.routes() == ((0, 0) if route == 2 else (1, 1)), (hint, counts.routes())
    assert counts.inner == len(counts.gathers), hint
    assert isinstance(out, distarray.DistArrayImpl) and out.tiles == arr.tiles and out.dtype == arr.dtype, hint
    np.testing.assert_array_equal(out.glom(), a + 1)
  counts.reset()
  out = blocks.map_blocks(_replicated(a), (1,), 0, plus_one)
  assert counts.routes() == (0, 0) and counts.inner == 0
  assert isinstance(out, distarray.ReplicatedArray)
  np.testing.assert_array_equal(out.glom(), a + 1)


def test_map_blocks_out_extent_and_target(blocks_ctx, counts):
  """A block that changes the shape: the result is cut where the caller says."""
  blocks_ctx(3)
  from spartan_amd.array import blocks, distarray, extent as ext
  a = _data()
  oshape = (6, 1)
  oext = lambda e: ext.create((e.ul[0], 0), (e.lr[0], 1), oshape)
  first = lambda t, shape: t[:, :1].contiguous()
  for hint, route in LAYOUTS:
    arr = _tiled(a, hint)
    counts.reset()
    out = blocks.map_blocks(arr, (1,), 0, first, out_shape=oshape, out_extent=oext,
                            target=lambda sl: blocks.deferred(oshape, arr.dtype, {oext(e): w for e, w in sl}))
    assert counts.routes() == ((0, 0) if route == 2 else (1, 1)), hint
    assert tuple(out.shape) == oshape and {(e.ul[0], e.lr[0]) for e in out.tiles} == \
        {(e.ul[0], e.lr[0]) for e in arr.tiles}, hint
    np.testing.assert_array_equal(out.glom(), a[:, :1])


def test_whole(blocks_ctx, counts):
  blocks_ctx(3)
  from spartan_amd.array import blocks
  a = _data()
  t = blocks.whole(_replicated(a))
  assert counts.gathers == [] and counts.exchanges == 0 and counts.inner == 0
  np.testing.assert_array_equal(t.numpy(), a)
  arr = _tiled(a, (3, 3))
  for ranks, n in ((None, 1), ({0}, 1), ({1, 0}, 2), ({1}, 1)):  # the context is rank 0 of a world of one
    counts.reset()
    t = blocks.whole(arr, ranks)
    assert counts.gathers == [n] and counts.exchanges == 0, ranks
    if ranks == {1}:
      assert t is None
    else:
      assert t.is_contiguous()
      np.testing.assert_array_equal(t.numpy(), a)


@pytest.mark.parametrize('W', [1, 3])
def test_sort_topk_maxpool_route_3(blocks_ctx, counts, W):
  """Each operation over a layout that needs the exchange: ONE gather of the
  data, ONE scatter."""
  blocks_ctx(W)
  from spartan_amd.expr.sort import sort_array
  from spartan_amd.expr.stencil import maxpool_array
  from spartan_amd.expr.topk import topk_array
  from stencil_ref import maxpool_ref
  a = _data()
  arr = _tiled(a, (6, 2))  # column strips: no tile holds a line of axis 1
  counts.reset()
  out = sort_array(arr, 1, False)
  print('sort: gathers %s, exchanges %d (+%d inside the gathers)' % (counts.gathers, counts.exchanges, counts.inner))
  assert counts.gathers == [1] and counts.exchanges == 1 and counts.inner == 1
  assert out.tiles == arr.tiles
  np.testing.assert_array_equal(out.glom(), np.sort(a, axis=1))
  counts.reset()
  out = sort_array(arr, 1, True)
  assert counts.gathers == [1] and counts.exchanges == 1 and out.dtype == np.int64
  np.testing.assert_array_equal(out.glom(), np.argsort(a, axis=1, kind='stable'))
  counts.reset()
  out = sort_array(arr, None, False)  # the flattened array: gathered whole to one owner
  print('sort(axis=None): gathers %s, exchanges %d' % (counts.gathers, counts.exchanges))
  assert counts.gathers == [1] and counts.exchanges == 1
  np.testing.assert_array_equal(out.glom(), np.sort(a, axis=None))
  counts.reset()
  out = topk_array(arr, 2, 1, False, False)
  print('topk: gathers %s, exchanges %d (+%d inside the gathers)' % (counts.gathers, counts.exchanges, counts.inner))
  assert counts.gathers == [1] and counts.exchanges == 1 and counts.inner == 1
  np.testing.assert_array_equal(out.glom(), np.sort(a, axis=1)[:, :2])
  img = _data((4, 2, 4, 4))
  planes = _tiled(img, (2, 2, 2, 4))  # cut along axis 0 and inside the planes: two slabs
  counts.reset()
  out = maxpool_array(planes, 2, 2)
  print('maxpool: gathers %s, exchanges %d (+%d inside the gathers)'
        % (counts.gathers, counts.exchanges, counts.inner))
  assert counts.gathers == [2] and counts.exchanges == 1 and counts.inner == 1
  assert sorted((e.ul, e.lr) for e in out.tiles) == [((0, 0, 0, 0), (2, 2, 2, 2)), ((2, 0, 0, 0), (4, 2, 2, 2))]
  np.testing.assert_array_equal(out.glom(), maxpool_ref(img, 2, 2))


@pytest.mark.parametrize('W', [1, 3])
def test_sort_routes_1_and_2(blocks_ctx, counts, W):
  blocks_ctx(W)
  from spartan_amd.array import distarray
  from spartan_amd.expr.sort import sort_array
  a = _data()
  for hint, route in LAYOUTS:
    arr = _tiled(a, hint)
    counts.reset()
    out = sort_array(arr, 1, False)
    assert counts.routes() == ((0, 0) if route == 2 else (1, 1)), (hint, counts.routes())
    np.testing.assert_array_equal(out.glom(), np.sort(a, axis=1))
  counts.reset()
  out = sort_array(_replicated(a), 1, False)
  assert counts.routes() == (0, 0) and isinstance(out, distarray.ReplicatedArray)
