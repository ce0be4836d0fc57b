"""Combine -- deliver: the route every operation takes that reduces into a
``DistArray`` (the fused map+reduce, ``dot``, the k-means joins, ``bincount``).
Every rank holds a full-size buffer -- a partial, or a result already identical
on all ranks -- that is combined over the ranks and cut into the output's tiles:

  * ``land``: the whole route for tile partials -- adopted where every one
    lands exactly on an output tile of its own rank, otherwise merged into one
    identity-filled buffer (``accumulate``) that goes ``across_ranks``;
  * ``across_ranks``: the ranks' buffers combined (RCCL reduce-scatter onto
    rank slabs, all-reduce otherwise; min / max and the arg-reductions by
    all-gather and a fold in rank order) and ``deliver``ed;
  * ``deliver``: a buffer identical on every rank into the local tiles.

The SPMD contract: everything here is decided from global metadata (shapes,
tile maps, worker ids), so every rank issues the same collectives in the same
order as long as callers call these functions on every rank.
"""
import numpy as np

from .. import backend, comm, runtime
from ..util import prod

# How many times each cross-rank combine ran (tests assert the branch taken).
COMBINE_CALLS = {'reduce_scatter': 0, 'all_reduce': 0, 'gather_combine': 0, 'arg_gather': 0}


def rank_slabs(output):
  """True iff output tiles are world_size equal row slabs, tile k on rank k."""
  ctx = runtime.get()
  if len(output.shape) == 0 or len(output.tiles) != ctx.world_size:
    return False
  exs = sorted(output.tiles.items(), key=lambda kv: kv[0].ul)
  n = exs[0][0].shape[0]
  for k, (ex, w) in enumerate(exs):
    if ctx.owner(w) != k or ex.ul[0] != k * n or ex.lr[0] - ex.ul[0] != n:
      return False
    if any(ex.ul[d] != 0 or ex.lr[d] != output.shape[d] for d in range(1, len(output.shape))):
      return False
  return True


def deliver(target, full):
  """A full-size tensor, identical on every rank, into target's local tiles.
  A local tile that IS the whole array and was never written adopts the tensor
  (no copy: the caller made it for this target alone); any other gets its
  region by one ``copy_region``."""
  be = backend.get()
  if len(target.local) == 1:
    (d, t), = target.local.items()
    if (not t.written and tuple(d.ul) == (0,) * len(target.shape) and tuple(d.shape) == tuple(target.shape)
        and tuple(full.shape) == tuple(t.shape) and full.dtype == backend.torch_dtype(target.dtype)):
      t.data = full if full.is_contiguous() else full.contiguous()
      t.written = [d]
      return
  for d, t in target.local.items():
    be.copy_region(t.data, (0,) * d.ndim, full, d.ul, d.shape)  # (0-d: all three are ())
    t.written = [d]


def _identity(op, dt):
  dt = np.dtype(dt)
  if op == 'sum':
    return 0.0
  if dt.kind == 'f':
    return float('inf') if op == 'min' else float('-inf')
  if dt.kind == 'b':
    return 1.0 if op == 'min' else 0.0
  info = np.iinfo(dt)
  return float(info.max) if op == 'min' else float(info.min)


def accumulate(shape, dtype, op, pieces):
  """The buffer of ``shape`` filled with op's identity, with ``pieces``
  ([(ul, tensor)]) merged into it in order (reference: output.update ->
  tile.merge with the reducer)."""
  import torch
  be = backend.get()
  full = torch.empty(shape, dtype=backend.torch_dtype(dtype), device=runtime.get().device)
  be.fill(full, backend.FILL_CONST, _identity(op, dtype), 0.0, 0, (0,) * len(shape), shape)
  for ul, t in pieces:
    be.merge(full, None, ul, t, op, fastpath=False)
  return full


def across_ranks(output, full, op):
  """Combine every rank's ``full`` with ``op`` ('sum', 'min', 'max') and
  deliver each output tile to its owner.  Collective."""
  import torch
  ctx = runtime.get()
  if ctx.distributed:
    if op != 'sum':
      # min / max across ranks: gather every rank's partial and fold them in
      # rank order with the local kernels' NaN rule (np.minimum / np.maximum
      # propagate NaN; the collective library's MIN / MAX need not)
      COMBINE_CALLS['gather_combine'] += 1
      stack = comm.all_gather_stack(full.reshape(-1))
      n = full.numel()
      folded = torch.empty((n,), dtype=full.dtype, device=full.device)
      backend.get().finalize(op, stack.reshape(-1), ctx.world_size, n, folded)
      full = folded.reshape(full.shape)
    elif rank_slabs(output):
      COMBINE_CALLS['reduce_scatter'] += 1
      (d, t), = output.local.items()
      comm.reduce_scatter_rows(t.data, full.contiguous(), op)
      t.written = [d]
      return
    else:
      COMBINE_CALLS['all_reduce'] += 1
      comm.all_reduce(full, op)
  deliver(output, full)


def across_ranks_arg(output, full_v, full_i, op):
  """``across_ranks`` for argmin / argmax: every rank's best values and their
  indices are gathered and the winner taken in rank order.  Collective."""
  if runtime.get().distributed:
    COMBINE_CALLS['arg_gather'] += 1
    vs = comm.all_gather_stack(full_v.reshape(-1))
    is_ = comm.all_gather_stack(full_i.reshape(-1))
    _, best_i = backend.get().argcombine(op, vs, is_)
    full_i = best_i.reshape(full_i.shape)
  deliver(output, full_i)


def _arg_merge_region(be, full_v, full_i, d, pv, pi, opname):
  import torch
  shape, ul = d.shape, d.ul
  n = prod(shape)
  old_v = torch.empty(shape, dtype=full_v.dtype, device=full_v.device)
  old_i = torch.empty(shape, dtype=torch.int64, device=full_v.device)
  be.copy_region(old_v, (0,) * len(shape), full_v, ul, shape)
  be.copy_region(old_i, (0,) * len(shape), full_i, ul, shape)
  pvc = pv.reshape(shape).to(full_v.dtype) if pv.dtype != full_v.dtype else pv.reshape(shape)
  vs = torch.stack([old_v.reshape(n), pvc.reshape(n)])
  is_ = torch.stack([old_i.reshape(n), pi.reshape(n)])
  bv, bi = be.argcombine(opname, vs, is_)
  be.copy_region(full_v, ul, bv.reshape(shape), (0,) * len(shape), shape)
  be.copy_region(full_i, ul, bi.reshape(shape), (0,) * len(shape), shape)


def _disjoint(dsts):
  """Are the extents pairwise disjoint?  (Sorted by ul: an extent is compared
  with those that start before it ends along axis 0.)"""
  ds = sorted(dsts, key=lambda d: d.ul)
  for i, a in enumerate(ds):
    for b in ds[i + 1:]:
      if a.ndim and b.ul[0] >= a.lr[0]:
        break
      if all(bu < al and au < bl for au, al, bu, bl in zip(a.ul, a.lr, b.ul, b.lr)):
        return False
  return True


def aligned(output, partials):
  """Does every partial land exactly on an output tile of its own rank, no two
  of them overlapping?  From global metadata: the same verdict on every rank."""
  ctx = runtime.get()
  for d, w, _ in partials:
    if d not in output.tiles or (w != -1 and ctx.owner(output.tiles[d]) != ctx.owner(w)):
      return False
  return _disjoint([d for d, _, _ in partials])


def land(output, partials, op, value_dtype=None):
  """Tile partials into ``output`` (reference: _reduce_mapper ->
  output.update(dst, partial) -> tile.merge with accumulate_fn).  Collective.

  ``partials``: [(destination extent, worker, tensor -- for argmin / argmax
  the pair (values, indices) -- or None where the partial is another rank's)]
  in tile order, the same list on every rank.  ``value_dtype``: for argmin /
  argmax, the dtype of the partial values (the same on every rank, also on
  ranks without a local partial)."""
  import torch
  be = backend.get()
  arg = op in ('argmin', 'argmax')
  mine = [(d, p) for d, _, p in partials if p is not None]
  if aligned(output, partials):
    for d, p in mine:
      t = output.local.get(d)
      if t is None:
        continue
      data = p[1] if arg else p
      tdt = backend.torch_dtype(t.dtype)
      if data.dtype != tdt:
        conv = torch.empty(t.shape, dtype=tdt, device=data.device)
        be.copy_region(conv, (0,) * conv.dim(), data, (0,) * conv.dim(), tuple(conv.shape))
        data = conv
      t.data = data if tuple(data.shape) == tuple(t.shape) else data.reshape(t.shape)
      t.written = [d]
    return
  shape = output.shape
  if not arg:
    full = accumulate(shape, output.dtype, op, [(d.ul, p.reshape(d.shape)) for d, p in mine])
    return across_ranks(output, full, op)
  # values keep their own dtype end to end: int64 compares as int64 (a
  # float64 detour would merge distinct values above 2^53)
  vdt = backend.torch_dtype(value_dtype) if value_dtype is not None else None
  for _, (pv, pi) in mine:
    vdt = pv.dtype
  if vdt is None:
    raise ValueError('land: value dtype of the arg-reduction unknown on this rank')
  ctx = runtime.get()
  full_v = torch.zeros(shape, dtype=vdt, device=ctx.device)
  full_i = torch.empty(shape, dtype=torch.int64, device=ctx.device)
  be.fill(full_i, backend.FILL_CONST, 9.3e18, 0.0, 0, (0,) * len(shape), shape)
  for d, (pv, pi) in mine:
    _arg_merge_region(be, full_v, full_i, d, pv, pi, op)
  across_ranks_arg(output, full_v, full_i, op)
