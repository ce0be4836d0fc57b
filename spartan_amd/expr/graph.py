"""``shortest_path``: all-pairs shortest path lengths on spx_apsp (DESIGN.md
3.23).

The reference's manifold learner (spartan/examples/sklearn/manifold/isomap.py)
runs a Cython Dijkstra per row tile.  Here the path metric of a graph is one
node: ``shortest_path(G, directed, unreachable)`` is the (n, n) array of path
lengths of the edge-weight matrix ``G``, computed by the blocked
Floyd-Warshall kernels of ``csrc/graph_kernels.h``.

The edge rules are the reference's (and scipy's for a dense graph): an
off-diagonal entry is an edge iff it is finite and > 0; ``0`` and ``+inf`` both
mean "no edge"; the diagonal is ignored and the result's diagonal is 0.  With
``directed=False`` the edge between i and j is the smaller of the edges
present in G[i, j] and G[j, i].  Where no path exists the result holds
``unreachable``.

``G`` may be a sparse array: this node is the one place besides ``dot``,
``todense`` and the sparse operations themselves that accepts a sparse
operand.  It is densified inside the node, slab by slab, through
``csr_todense`` (a stored zero is "no edge" like an absent entry), and the
result is tiled in row slabs at the input's row cuts.

Routes; every rank issues the same exchanges whether or not it owns tiles:

  * a replicated array, or an array in one tile, is computed on its holder;
  * any other layout is gathered to one owner (it must fit that GPU), computed
    there and delivered into the input's tiling by one ``scatter_slabs``
    (``array/blocks.py``).

``info`` of the kernel stays on the device until the end of the evaluation; the
smallest value over all ranks is then read once, and a negative one raises
``ValueError('shortest_path: negative or NaN edge weight')`` on every rank.

Not built: predecessors / path reconstruction, negative weights, a result
distributed across GPUs during the computation.
"""
import numpy as np

from .. import backend, comm, runtime
from ..array import distarray
from ..array.blocks import deferred, gather_slabs, scatter_slabs, with_tiles
from .base import Expr, as_array

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


class ShortestPathExpr(Expr):
  _members = ('array',)
  accepts_sparse = True

  def compute_shape(self):
    return self.array.shape

  def compute_dtype(self):
    return np.dtype(self.array.dtype)

  def pretty_str(self):
    return 'ShortestPath[%d](%s, directed=%s, unreachable=%r)' % (self.expr_id, self.array, self.directed,
                                                                  self.unreachable)

  def _evaluate(self, deps):
    from .sparse import todense_array
    arr = deps['array']
    if getattr(arr, 'sparse', False):
      arr = todense_array(arr)
    return shortest_path_array(distarray.as_array(arr), self.directed, self.unreachable)


def shortest_path(G, directed=True, unreachable=np.inf):
  """The (n, n) array of shortest path lengths of the graph whose edge weights
  are the float32 / float64 matrix ``G``, lazily, in G's dtype.  ``G`` is a
  dense array or expression, or a sparse array (densified inside the node).
  An off-diagonal entry is an edge iff it is finite and > 0; 0, +inf and a
  stored zero mean "no edge".  ``directed=False`` takes the smaller of the
  edges present in G[i, j] and G[j, i].  Pairs without a path get
  ``unreachable``.  Evaluation raises ``ValueError`` for a negative or NaN
  weight."""
  from .sparse import as_sparse_expr, is_sparse
  G = as_sparse_expr(G) if is_sparse(G) else as_array(G)
  shape = tuple(G.shape)
  if len(shape) != 2 or shape[0] != shape[1]:
    raise ValueError('shortest_path: a square 2-d array is needed, got shape %s' % (shape,))
  dt = np.dtype(G.dtype)
  if dt not in _FLOATS:
    raise TypeError('shortest_path: dtype %s is not float32 / float64' % dt)
  unreachable = float(unreachable)
  if not unreachable >= 0.0:
    raise ValueError('shortest_path: unreachable = %r is negative or NaN' % unreachable)
  node = ShortestPathExpr(array=G)
  node.directed = bool(directed)
  node.unreachable = unreachable
  return node


# ------------------------------------------------------------- evaluation
def _raise_on_info(infos):
  """``infos``: the info tensors of this rank's apsp calls.  The smallest entry
  over all ranks is read (the evaluation's one host read); a negative one
  raises.  Collective."""
  import torch
  ctx = runtime.get()
  worst = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
  for info in infos:
    worst = torch.minimum(worst, info.to(torch.int64).min().reshape(1))
  worst = comm.all_reduce(worst, 'min')
  if int(worst.item()) < 0:
    raise ValueError('shortest_path: negative or NaN edge weight')


def _block(t, directed, unreachable, infos):
  be = backend.get()
  D, info = be.apsp(be.contiguous(t), directed, unreachable)
  infos.append(info)
  return D


def shortest_path_array(arr, directed=True, unreachable=np.inf):
  """The path-length array of the dense array ``arr``."""
  ctx = runtime.get()
  arr = with_tiles(arr)
  infos = []
  if arr.replicated:  # held in full by every rank
    D = _block(arr.device_data(), directed, unreachable, infos)
    _raise_on_info(infos)
    return distarray.ReplicatedArray(D)
  if len(arr.tiles) == 1:
    (e, w), = arr.tiles.items()
    local = {}
    if ctx.is_local(w):
      local[e] = _block(arr.fetch(e), directed, unreachable, infos)
    _raise_on_info(infos)
    return distarray.from_tiles(arr.shape, arr.dtype, arr.tiles, local)
  sl, got = gather_slabs(arr, None)  # the whole matrix on the owner of its first tile
  target = deferred(arr.shape, arr.dtype, arr.tiles)
  scatter_slabs(target, sl, {qi: _block(t, directed, unreachable, infos) for qi, t in got.items()})
  _raise_on_info(infos)
  return target
