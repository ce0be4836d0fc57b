"""The reference's k-means driver, runnable unmodified on the MI355X path
(spartan/examples/sklearn/cluster/k_means_.py).

``KMeans.fit(X, centers, implementation='outer')`` is the reference's loop
(k_means_.py:108-152) written against ``expr.outer`` / ``expr.argmin`` /
``expr.map2`` with the reference's three mapper functions.  Those mappers
are registered joins (expr/join.py), so each runs as device work:

  kmeans_dist_mapper    outer((X, C), (0, 0))  -> spx_cdist: exact-order fp64
                        distances (N, K), rounded to the target dtype;
  argmin(outer(...), axis=1)                   -> fused by OuterArgminFusion
                        (expr/optimize.py) into spx_kmeans_assign for fp64
                        or fp32 distances (the argmin of the values rounded to
                        the target dtype): certified bf16x3-MFMA filter +
                        exact recompute, no (N, K) matrix (102-205 GB at cfg3);
                        in spx_kmeans_step's domain the fused step, whose
                        centre sums / counts the two joins below then take
                        (one pass over X per iteration);
  kmeans_count_mapper   map2(labels, 0)        -> spx_bincount per label tile
                        + RCCL all-reduce;
  kmeans_center_mapper  map2((X, labels), (0, 0)) -> spx_kmeans_accumulate
                        per-centre fp64 sums + RCCL all-reduce.

The mapper bodies below are the host meaning of each join (the reference's
NumPy code, restated); they are never called on the product path.

Divergence kept from workloads.kmeans_fit: counts and
centre sums are SUMMED over tiles, where the reference's reducer-less map2
keeps the last tile's; empty clusters are reseeded from a
seeded generator instead of the global ``np.random``.
"""
import os
import types
import weakref

import numpy as np

from .. import backend, comm, expr, runtime
from ..array import blocks, combine, distarray, extent as ext, transfer
from ..expr.join import register_argmin_fusion, register_join


# ------------------------------------------------------ the three mappers
def kmeans_dist_mapper(ex_a, tile_a, ex_b, tile_b):
  """k_means_.py:52-58: cdist of a point tile against a centre tile."""
  from scipy.spatial.distance import cdist
  target_ex = ext.create((ex_a.ul[0], ex_b.ul[0]), (ex_a.lr[0], ex_b.lr[0]),
                         (ex_a.array_shape[0], ex_b.array_shape[0]))
  yield target_ex, cdist(tile_a, tile_b)


def kmeans_count_mapper(extents, tiles, centers_count):
  """k_means_.py:61-64: np.bincount of a label tile."""
  target_ex = ext.create((0,), (centers_count,), (centers_count,))
  yield target_ex, np.bincount(tiles[0].astype(np.int64), minlength=centers_count)


def kmeans_center_mapper(extents, tiles, centers_count):
  """k_means_.py:67-89: per-centre sums of the points carrying each label."""
  points, labels = tiles
  target_ex = ext.create((0, 0), (centers_count, points.shape[1]), (centers_count, points.shape[1]))
  new_centers = np.zeros((centers_count, points.shape[1]))
  for i in range(centers_count):
    new_centers[i] = points[labels == i].sum(axis=0)
  yield target_ex, new_centers


# -------------------------------------------------------- device joins
def _replicated_f64(array):
  """The whole ``array`` as a contiguous fp64 tensor on every rank (collective)."""
  ctx = runtime.get()
  full = ext.from_shape(array.shape)
  got = distarray.gather_regions(array, [(full, r) for r in range(ctx.world_size)])
  return backend.get().contiguous(got[ctx.rank], np.float64)


def _row_blocks(X, ncols):
  """[(owner rank, row extent over all columns)] of X's row blocks, and
  {index: device tensor} of the local ones (gathered when X is column-split).
  Kept across iterations at world size 1 (_PIPE.rows: an iterative driver passes
  the same forced X every time; with more ranks the gather is a collective
  every rank must enter, so nothing is cached)."""
  ctx = runtime.get()
  local = getattr(X, 'local', None)
  tiles = None
  if ctx.world_size == 1 and isinstance(local, dict) and not getattr(X, 'replicated', False):
    tiles = [(tuple(ex.ul), t._data) for ex, t in local.items()]
    hit = _PIPE.rows
    if (hit is not None and hit[0]() is X and hit[1] == ncols and len(hit[2]) == len(tiles)
        and all(a[0] == b[0] and a[1] is b[1] for a, b in zip(hit[2], tiles))):
      return hit[3], hit[4]
  rows = sorted({(ex.ul[0], ex.lr[0]): w for ex, w in X.tiles.items()}.items())
  blocks = [(ctx.owner(w) if w != -1 else ctx.rank,
             ext.create((r0, 0), (r1, ncols), X.shape) if len(X.shape) == 2 else ext.create((r0,), (r1,), X.shape))
            for (r0, r1), w in rows]
  got = distarray.gather_regions(X, [(region, dst) for dst, region in blocks])
  _PIPE.rows = None if tiles is None else (weakref.ref(X, _PIPE.drop_rows), ncols, tiles, blocks, got)
  return blocks, got


def _local_rows(X, ncols):
  """X's row blocks (_row_blocks; collective), and an iterator over this
  rank's: (index, region, the block's points with unit column stride)."""
  rank, be = runtime.get().rank, backend.get()
  blocks, got = _row_blocks(X, ncols)
  mine = ((qi, region, got[qi]) for qi, (src, region) in enumerate(blocks) if src == rank)
  return blocks, ((qi, region, p if p.stride(-1) == 1 else be.contiguous(p)) for qi, region, p in mine)


def _dist_join(kind, arrays, axes, fn_kw, target):
  import torch
  if kind != 'outer' or tuple(axes) != (0, 0) or len(arrays[0].shape) != 2:
    raise NotImplementedError('kmeans_dist_mapper: outer((X, C), (0, 0)) over a 2-d X only')
  X, C = arrays
  ctx = runtime.get()
  be = backend.get()
  c = _replicated_f64(C)
  K, D = c.shape
  row_blocks, rows = _local_rows(X, D)
  dist = {}
  for qi, region, pts in rows:
    dist[qi] = torch.empty((region.shape[0], K), dtype=backend.torch_dtype(target.dtype), device=ctx.device)
    be.cdist(pts, c, dist[qi])
  blocks.scatter_updates(target, [(qi, ext.create((r.ul[0], 0), (r.lr[0], K), target.shape), src, dist.get(qi))
                                  for qi, (src, r) in enumerate(row_blocks)])


def _count_join(kind, arrays, axes, fn_kw, target):
  import torch
  ctx = runtime.get()
  be = backend.get()
  K = int(fn_kw['centers_count'])
  labels = arrays[0]
  pre = _PIPE.take(labels, K)
  if pre is not None:
    comm.all_reduce(pre, 'sum')
    combine.deliver(target, pre)
    _PIPE.counts_delivered(target)
    return
  counts = torch.zeros((K,), dtype=torch.int64, device=ctx.device)
  for ex, tile in labels.local.items():
    lab = be.contiguous(tile.data, np.int64).reshape(-1)
    be.bincount(lab, counts, zero_first=False)
  comm.all_reduce(counts, 'sum')
  combine.deliver(target, counts)


def _center_join(kind, arrays, axes, fn_kw, target):
  import torch
  ctx = runtime.get()
  be = backend.get()
  K = int(fn_kw['centers_count'])
  X, labels = arrays
  D = X.shape[1]
  pre = _PIPE.take(labels, K, X)
  if pre is not None:  # the fused step of this labels array already summed X
    comm.all_reduce(pre, 'sum')
    combine.deliver(target, pre)
    _PIPE.sums_delivered(X, K, target)
    return
  sums = torch.zeros((K, D), dtype=torch.float64, device=ctx.device)
  counts = torch.zeros((K,), dtype=torch.int64, device=ctx.device)
  blocks, rows = _local_rows(X, D)
  lab_blocks = distarray.gather_regions(labels, [(ext.create((r.ul[0],), (r.lr[0],), labels.shape)
                                                  if len(labels.shape) == 1 else
                                                  ext.create((r.ul[0], 0), (r.lr[0], labels.shape[1]), labels.shape),
                                                  dst) for dst, r in blocks])
  for qi, _region, pts in rows:
    lab = be.contiguous(lab_blocks[qi], np.int64).reshape(-1)
    be.kmeans_accumulate(pts, lab, sums, counts, zero_first=False)
  comm.all_reduce(sums, 'sum')
  combine.deliver(target, sums)


def _step_domain(X, K):
  """True where spx_kmeans_step fuses (fp32 rows of 64 / 128 dims, K <= 256,
  row-strip tiles): decided from global metadata, so every rank agrees."""
  return (np.dtype(X.dtype) == np.float32 and len(X.shape) == 2 and X.shape[1] in (64, 128) and K <= 256
          and all(ex.ul[1] == 0 and ex.lr[1] == X.shape[1] for ex in X.tiles))


def _assign_fused(arrays, fn_kw, target, dist_dtype):
  """argmin(outer((X, C), (0, 0), kmeans_dist_mapper), axis=1): the outer's
  target holds the cdist values rounded to its dtype (fp64, or fp32 for fp32
  points: map2 / outer dtype None -> arrays[0].dtype); spx_kmeans_assign per
  X row block gives the argmin of exactly those values (first index on
  ties, first NaN wins) without materialising them.  In spx_kmeans_step's
  domain the same labels come from the fused step, whose centre sums and
  counts (of the same single pass over X) the centre / count joins of THAT
  labels array over THAT X take (_PIPE.hand_off) instead of reading X again."""
  import torch
  X, C = arrays
  ctx = runtime.get()
  be = backend.get()
  c = _replicated_f64(C)
  K, D = c.shape
  row_blocks, rows = _local_rows(X, D)
  fused = _step_domain(X, K)
  spec = _PIPE.take_queued(X, K, c, dist_dtype) if fused else None
  if spec is not None:  # the step queued for these very centres (_speculate)
    labs, sums, counts = spec.labs, spec.sums, spec.counts
  elif fused:
    labs, sums, counts = _fused_step(rows, c, dist_dtype)
  else:
    labs = {}
    for qi, region, pts in rows:
      labs[qi] = torch.empty((region.shape[0],), dtype=torch.int64, device=ctx.device)
      be.kmeans_assign(pts, c, labs[qi], dist_dtype=dist_dtype)
  blocks.scatter_updates(target, [(qi, ext.create((r.ul[0],), (r.lr[0],), target.shape), src, labs.get(qi))
                                  for qi, (src, r) in enumerate(row_blocks)])
  if fused:
    _PIPE.hand_off(X, target, K, sums, counts, dist_dtype, adopted=spec is not None)


def _fused_step(rows, c, dist_dtype):
  """spx_kmeans_step for centres c (device fp64) over this rank's row blocks (rows:
  _local_rows), in fresh buffers: ({block index: labels}, centre sums, counts)."""
  import torch
  be = backend.get()
  # the first local block's step writes them (zero_first), the others add
  sums = torch.empty(tuple(c.shape), dtype=torch.float64, device=c.device)
  counts = torch.empty((c.shape[0],), dtype=torch.int64, device=c.device)
  labs = {}
  for qi, _region, pts in rows:
    lab = torch.empty((pts.shape[0],), dtype=torch.int64, device=c.device)
    be.kmeans_step(pts, c, lab, sums, counts, zero_first=not labs, dist_dtype=dist_dtype)
    labs[qi] = lab
  if not labs:  # no local row block on this rank
    sums.zero_()
    counts.zero_()
  return labs, sums, counts


# Speculation (world size 1; SPARTAN_KMEANS_SPECULATE, default on).  The
# reference's loop reads the counts and the centre sums back to the host,
# divides there and uploads the new centres (k_means_.py:140-150): the GPU
# idles for that round trip and for the building of the next iteration's
# expressions.  While KMeans.fit has an iteration to go (following), the centre
# join, once the sums are all-reduced and delivered, (1) computes the next
# centres on the device exactly as the host will (the sums and counts rounded
# to the joins' target dtypes, divided in NumPy's result dtype), (2) copies
# the delivered sums to pinned memory and attaches that copy as the host
# shadow of the target tile (array/transfer.py), so the host's glom does not
# wait behind (3), the next fused step queued on the same stream with those
# centres.  The next fused assignment adopts that step's labels, sums and
# counts only if ITS centres are bit-identical to the queued ones (compared
# on the device); an empty cluster (reseeded on the host) or any other
# centres run the step as usual, after the queued one.  Results are those of
# the sequential loop.  (A side stream cannot overlap: k_kmeans_pp holds every
# CU's register file and LDS, so any other kernel -- the runtime's copy
# kernels too -- waits for it.)
SPEC_STATS = {'queued': 0, 'adopted': 0, 'dropped': 0}


def _spec_on():
  ctx = runtime.get()
  return (ctx.world_size == 1 and ctx.device.type == 'cuda'
          and os.environ.get('SPARTAN_KMEANS_SPECULATE', '1') != '0')


class _Pinned:
  """One pinned staging buffer, and the device tensor whose host shadow or
  upload alias (array/transfer.py) reads from it until somebody takes it."""
  buf = lent = None

  def stage(self, t):
    """Start t's copy into the buffer (withdrawing what still reads from it): its host view."""
    import torch
    self.withdraw()
    if self.buf is None or tuple(self.buf.shape) != tuple(t.shape) or self.buf.dtype != t.dtype:
      self.buf = torch.empty(tuple(t.shape), dtype=t.dtype, pin_memory=True)
    self.buf.copy_(t, non_blocking=True)
    return self.buf.numpy()

  def withdraw(self):
    transfer.drop_shadow(self.lent)  # (each drops an entry for THIS tensor only)
    transfer.drop_upload_alias(self.lent)
    self.lent = None


class _Pipeline:
  """What the four joins hand to each other and to KMeans.fit.  One instance
  (_PIPE): the joins are registered callbacks, and a loop written by hand
  gets the same one-pass hand-off as KMeans.fit.  X and the label arrays are
  referred to weakly only: nothing here extends their lives."""

  def __init__(self):
    # for the process (reset() keeps them: a warm-up fit pays for them)
    self.pin_sums, self.pin_counts, self.pin_centres = _Pinned(), _Pinned(), _Pinned()
    # the row-block cache, one entry (weak X, ncols, [(tile origin, tile tensor)],
    # blocks, rows): valid while X lives and every local tile tensor is the same
    # object (the rows are views of them); reset() keeps it for the next fit of X
    self.rows = None
    self.reset()

  def reset(self):
    """Drop one iteration's hand-off and the queued step and withdraw what was
    registered here and never taken (KMeans.fit: on entry, and however it ends)."""
    # the last fused assignment's per-rank centre sums and counts, each taken
    # once by the join of THAT labels array (over THAT X)
    self.step_X = self.step_labels = self.step_K = self.step_dd = self.step_sums = self.step_counts = None
    self.red_counts = None  # its all-reduced counts as the host will read them (count join -> _speculate)
    # the dtypes the count / centre joins delivered in (the host reads them so)
    self.sums_dtype = self.counts_dtype = None
    # (host copy, event) staged by _speculate_early for this iteration's joins
    self.early_sums = self.early_counts = None
    # the queued step (weak X, K, distance dtype, centres cn, {block index:
    # labels}, sums, counts), until the next assignment takes or drops it
    self.queued = None
    self.following = False  # "another iteration follows": set by KMeans.fit around its two gloms
    for pin in (self.pin_sums, self.pin_counts, self.pin_centres):
      pin.withdraw()

  def drop_rows(self, _ref):
    self.rows = None  # (the cached X died)

  def hand_off(self, X, labels, K, sums, counts, dd, adopted):
    """From the fused assignment: this rank's sums and counts of (X, labels)."""
    self.step_X, self.step_labels = weakref.ref(X), weakref.ref(labels)
    self.step_K, self.step_dd, self.step_sums, self.step_counts = K, dd, sums, counts
    self.early_sums = self.early_counts = self.red_counts = None
    if adopted and _spec_on():
      self._speculate_early(X, K, sums, counts, dd)

  def take(self, labels, K, X=None):
    """This rank's fused counts for labels (given X: the centre sums for (X, labels)), once each, or None."""
    if self.step_labels is None or self.step_labels() is not labels or self.step_K != K \
        or X is not None and self.step_X() is not X:
      return None
    if X is None:
      pre, self.step_counts = self.step_counts, None
    else:
      pre, self.step_sums = self.step_sums, None
    return pre

  def counts_delivered(self, target):
    self.counts_dtype = np.dtype(target.dtype)
    self._early_shadow(self.pin_counts, self.early_counts, target)
    self.early_counts = None
    if len(target.local) == 1:  # the counts as the host will read them, for _speculate
      (_ex, tile), = target.local.items()
      self.red_counts = tile.data

  def sums_delivered(self, X, K, target):
    self.sums_dtype = np.dtype(target.dtype)
    self._early_shadow(self.pin_sums, self.early_sums, target)
    self.early_sums = None
    if self.following and self.queued is None:  # (not queued early, _speculate_early)
      self._speculate(X, K, target)

  def _early_shadow(self, pin, staged, target):
    """Attach the early-staged host copy to target's tile (if dtype and shape match what was staged)."""
    if staged is None or len(target.local) != 1:
      return
    host, ev = staged
    (_ex, tile), = target.local.items()
    tt = tile.data
    if np.dtype(target.dtype) == host.dtype and tuple(tt.shape) == tuple(host.shape):
      transfer.attach_shadow(tt, host, ev)
      pin.lent = tt

  def _speculate(self, X, K, target):
    """At the centre join (no step queued yet: the loop's first iteration, or
    after a dropped one): queue the next step behind a pinned copy of the sums
    the host is about to glom (a host shadow of the target tile)."""
    if not _spec_on() or self.red_counts is None or len(target.local) != 1:
      return
    counts, self.red_counts = self.red_counts, None
    (_ex, tile), = target.local.items()
    tt = tile.data  # the centre sums as the host will read them (the target's dtype)
    if tuple(tt.shape) != (K, X.shape[1]) or tuple(counts.shape) != (K,):
      return
    self._stage(X, K, tt, counts, self.step_dd, shadow_now=True, queue=True)

  def _speculate_early(self, X, K, sums, counts, dd):
    """At the adoption of a queued step (world size 1: its sums and counts ARE the
    values this iteration's joins deliver): queue the step after it right away,
    computing its centres as the host will (the joins' target dtypes of the last
    iteration, NumPy's result dtype), and stage pinned copies of what the host will
    glom -- the counts, the sums in the centre target's dtype -- and of those centres,
    all before the step, so that neither the gloms nor the upload of the centres wait
    behind it.  The joins attach the copies as host shadows of their target tiles."""
    if self.sums_dtype is None or self.counts_dtype is None:
      return
    # (the loop's last iteration queues nothing, but still stages the copies: its gloms
    # and the upload of the final centres then need no round trip of their own)
    st, ct = sums.to(backend.torch_dtype(self.sums_dtype)), counts.to(backend.torch_dtype(self.counts_dtype))
    self._stage(X, K, st, ct, dd, shadow_now=False, queue=self.following)

  def _stage(self, X, K, st, ct, dd, shadow_now, queue):
    """The next centres from sums st / counts ct (device, in the dtypes the joins
    deliver), divided as the host will; pinned copies of st (its shadow now, or
    staged with ct's for the joins to attach) and of the centres; then the step."""
    import torch
    rdt = backend.torch_dtype(np.result_type(backend.np_dtype(st.dtype), backend.np_dtype(ct.dtype)))
    cn = (st.to(rdt) / ct.to(rdt).view(K, 1)).to(torch.float64)
    hs = self.pin_sums.stage(st)
    hk = None if shadow_now else self.pin_counts.stage(ct)
    # the centres the host will compute, to host too: its from_numpy of them
    # then takes cn itself instead of a synchronous upload queued behind the
    # step (transfer.register_upload_alias; bit-identical or not taken)
    hc = self.pin_centres.stage(cn)
    ev = torch.cuda.Event()
    ev.record()
    if shadow_now:
      transfer.attach_shadow(st, hs, ev)
      self.pin_sums.lent = st
    else:
      self.early_sums, self.early_counts = (hs, ev), (hk, ev)
    transfer.register_upload_alias(hc, cn, ev)
    self.pin_centres.lent = cn
    if queue:
      labs, sums, counts = _fused_step(_local_rows(X, X.shape[1])[1], cn, dd)  # on the current stream
      self.queued = types.SimpleNamespace(X=weakref.ref(X), K=K, dd=dd, cn=cn, labs=labs, sums=sums, counts=counts)
      SPEC_STATS['queued'] += 1

  def take_queued(self, X, K, c, dist_dtype):
    """The queued step if it ran for exactly these centres (bit for bit), X, K
    and distance dtype, else None."""
    import torch
    sp, self.queued = self.queued, None
    if sp is None:
      return None
    # (the comparison's host sync waits for the queued step: the GPU is busy)
    if not (sp.X() is X and sp.K == K and sp.dd == dist_dtype and tuple(c.shape) == tuple(sp.cn.shape)
            and torch.equal(c.contiguous().view(torch.int64), sp.cn.view(torch.int64))):
      SPEC_STATS['dropped'] += 1
      return None
    SPEC_STATS['adopted'] += 1
    return sp


_PIPE = _Pipeline()


register_join(kmeans_dist_mapper, _dist_join)
register_argmin_fusion(kmeans_dist_mapper, _assign_fused, dtypes=(np.float64, np.float32))
register_join(kmeans_count_mapper, _count_join)
register_join(kmeans_center_mapper, _center_join)


# --------------------------------------------------------------- KMeans
class KMeans(object):
  """k_means_.py:90-152."""

  def __init__(self, n_clusters=8, n_iter=100, seed=0):
    self.n_clusters = n_clusters
    self.n_iter = n_iter
    self.seed = seed

  def fit(self, X, centers=None, implementation='outer'):
    """X: (N, D) array tiled by rows; centers: (K, D) host array / Expr, or
    None (``expr.rand``).  Returns (centers (K, D) host fp64, labels)."""
    if implementation == 'broadcast':
      return self._fit_broadcast(X, centers)
    if implementation != 'outer':
      raise NotImplementedError('implementation %r: "outer" (default) and "broadcast" are on the path'
                                % implementation)
    _PIPE.reset()
    try:
      num_dim = X.shape[1]
      rng = np.random.default_rng(self.seed)
      labels = expr.zeros((X.shape[0], 1), dtype=np.int64)
      if centers is None:
        centers = expr.rand(self.n_clusters, num_dim)
      elif isinstance(centers, np.ndarray):
        centers = expr.from_numpy(centers)
      for i in range(self.n_iter):
        self.assign_centers_ = centers  # the centres this iteration's labels are assigned against
        distances = expr.outer((X, centers), (0, 0), fn=kmeans_dist_mapper,
                               shape=(X.shape[0], centers.shape[0]))
        labels = expr.argmin(distances, axis=1)
        counts = expr.map2(labels, 0, fn=kmeans_count_mapper, fn_kw={'centers_count': self.n_clusters},
                           shape=(centers.shape[0],))
        new_centers = expr.map2((X, labels), (0, 0), fn=kmeans_center_mapper,
                                fn_kw={'centers_count': self.n_clusters},
                                shape=(centers.shape[0], centers.shape[1]))
        # (another iteration follows: the centre join may queue it, _speculate;
        # if a glom raises, fit's reset() lowers the flag)
        _PIPE.following = i + 1 < self.n_iter
        counts = counts.optimized().glom()
        centers = new_centers.optimized().glom()
        _PIPE.following = False
        zcount_indices = (counts == 0).reshape(self.n_clusters)
        if np.any(zcount_indices):
          n_points = np.count_nonzero(zcount_indices)
          counts[zcount_indices] = 1
          centers[zcount_indices, :] = rng.standard_normal((n_points, num_dim))
        centers = centers / counts.reshape(centers.shape[0], 1)
        centers = expr.from_numpy(centers)
      return centers.glom(), labels
    finally:  # nothing of this fit outlives it (X, its labels, a queued step, untaken shadows)
      _PIPE.reset()

  def _fit_broadcast(self, X, centers):
    """k_means_.py:153-187: the same iteration written with broadcasting
    only -- (N, 1, D) - (1, K, D) squared and summed over the last axis (one
    fused map+reduce over the (N, K, D) iteration space, never
    materialised), argmin, one-hot matches by ``==`` against an arange,
    counts and centre sums as axis-0 reductions of broadcast products.  The
    distances are squared sums in the points' dtype (no sqrt, no fp64
    cdist), so near-tie labels follow this float order, as in the reference."""
    num_dim = X.shape[1]
    rng = np.random.default_rng(self.seed)
    if centers is None:
      centers = expr.rand(self.n_clusters, num_dim)
    elif isinstance(centers, np.ndarray):
      centers = expr.from_numpy(centers)
    labels = None
    for i in range(self.n_iter):
      X_broadcast = expr.reshape(X, (X.shape[0], 1, X.shape[1]))
      centers_broadcast = expr.reshape(centers, (1, centers.shape[0], centers.shape[1]))
      distances = expr.sum(expr.square(X_broadcast - centers_broadcast), axis=2)
      labels = expr.argmin(distances, axis=1)
      center_idx = expr.arange((1, centers.shape[0]))
      matches = expr.reshape(labels, (labels.shape[0], 1)) == center_idx
      matches = matches.astype(np.int64)
      counts = expr.sum(matches, axis=0)
      centers = expr.sum(X_broadcast * expr.reshape(matches, (matches.shape[0], matches.shape[1], 1)), axis=0)
      counts = counts.optimized().glom()
      centers = centers.optimized().glom()
      zcount_indices = (counts == 0).reshape(self.n_clusters)
      if np.any(zcount_indices):
        n_points = np.count_nonzero(zcount_indices)
        counts[zcount_indices] = 1
        centers[zcount_indices, :] = rng.standard_normal((n_points, num_dim))
      centers = centers / counts.reshape(centers.shape[0], 1)
      centers = expr.from_numpy(centers)
    return centers.glom(), labels
