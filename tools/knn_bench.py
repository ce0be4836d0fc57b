"""Times the fused nearest-neighbour search and the selection kernels against
the routes the same answers took before they existed:

  knn   spx_knn (distances + selection + the combine of the point ranges)
        vs spx_cdist into a distance matrix, spx_sort for values and indices,
        and a slice;
  topk  spx_topk vs spx_sort + slice.

One GPU, one process per leg (each under its own time limit), HIP events after
warm-up, the median of the timed repeats.  Prints one JSON line per leg and a
final summary line; ``--out FILE`` also writes them to FILE.

  python tools/knn_bench.py [--out profiles/knn_bench.json] [--reps 5]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_OPS_PER_S = 78.6e12 / 2  # vector fp64: 78.6 TF/s counts an FMA as two; sub / mul / add are one each
HBM_BYTES_PER_S = 6.29e12     # measured streaming read (float4 copy)

KNN_SHAPES = [dict(Q=4096, N=1 << 20, D=64, k=10), dict(Q=16, N=1 << 24, D=16, k=10)]
TOPK_SHAPES = [dict(outer=4096, n=(1 << 20) // 4, inner=1, k=10), dict(outer=8, n=1 << 24, inner=1, k=10)]
LEGS = ['knn_fused:0', 'knn_parent:0', 'knn_fused:1', 'knn_parent:1',
        'topk_select:0', 'topk_sort:0', 'topk_select:1', 'topk_sort:1']
LIMIT_S = {'knn_parent:0': 420}


def _time(fn, reps):
  import torch
  fn()
  torch.cuda.synchronize()
  ms = []
  for _ in range(reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    ms.append(a.elapsed_time(b))
  ms.sort()
  return ms[len(ms) // 2], ms


def run_leg(leg, reps):
  import numpy as np
  import torch
  import spartan_amd
  from spartan_amd import backend
  spartan_amd.initialize()
  be = backend.get()
  name, si = leg.split(':')
  si = int(si)
  g = torch.Generator(device='cuda').manual_seed(1234 + si)
  res = {'leg': leg}
  if name.startswith('knn'):
    s = KNN_SHAPES[si]
    Q, N, D, k = s['Q'], s['N'], s['D'], s['k']
    X = torch.rand((N, D), dtype=torch.float32, device='cuda', generator=g)
    q32 = torch.rand((Q, D), dtype=torch.float32, device='cuda', generator=g)
    q = q32.double()
    out_s = torch.empty((Q, k), dtype=torch.float64, device='cuda')
    out_i = torch.empty((Q, k), dtype=torch.int64, device='cuda')
    res.update(s, dtype='float32')
    if name == 'knn_fused':
      med, all_ms = _time(lambda: be.knn(X, q, k, 0, out_s, out_i), reps)
      bound_ms = 3.0 * Q * N * D / FP64_OPS_PER_S * 1e3
      res.update(ms=med, all_ms=all_ms, fp64_valu_bound_ms=bound_ms, fraction_of_fp64_valu_bound=bound_ms / med,
                 ranges=backend.knn_plan(Q, N, D, k)[0])
    elif Q > 64:
      # the (Q, N) matrix in batches of queries (the whole one, its sort buffers and
      # the int64 indices would not fit): queries as cdist's points, X as its fp64 centres
      QB = 256
      Xd = X.double()
      mat = torch.empty((QB, N), dtype=torch.float32, device='cuda')
      sv, si64 = torch.empty_like(mat), torch.empty((QB, N), dtype=torch.int64, device='cuda')
      dist = torch.empty((Q, k), dtype=torch.float32, device='cuda')

      def parent():
        for b0 in range(0, Q, QB):
          be.cdist(q32[b0:b0 + QB], Xd, mat)
          be.sort(mat, sv, si64, (QB, N, 1))
          dist[b0:b0 + QB] = sv[:, :k]
          out_i[b0:b0 + QB] = si64[:, :k]
      med, all_ms = _time(parent, min(reps, 2))
      res.update(ms=med, all_ms=all_ms, route='cdist (%d, N) + sort(values, indices) + slice, %d batches'
                 % (QB, Q // QB))
    else:
      # X as cdist's points, the queries as its centres: an (N, Q) matrix sorted along axis 0
      mat = torch.empty((N, Q), dtype=torch.float32, device='cuda')
      sv, si64 = torch.empty_like(mat), torch.empty((N, Q), dtype=torch.int64, device='cuda')
      dist = torch.empty((k, Q), dtype=torch.float32, device='cuda')

      def parent():
        be.cdist(X, q, mat)
        be.sort(mat, sv, si64, (1, N, Q))
        dist.copy_(sv[:k])
        out_i.copy_(si64[:k].t())
      med, all_ms = _time(parent, reps)
      res.update(ms=med, all_ms=all_ms, route='cdist (N, Q) + sort(values, indices) along axis 0 + slice')
  else:
    s = TOPK_SHAPES[si]
    o, n, i, k = s['outer'], s['n'], s['inner'], s['k']
    x = torch.rand((o, n, i), dtype=torch.float32, device='cuda', generator=g)
    res.update(s, dtype='float32')
    if name == 'topk_select':
      v = torch.empty((o, k, i), dtype=torch.float32, device='cuda')
      idx = torch.empty((o, k, i), dtype=torch.int64, device='cuda')
      med, all_ms = _time(lambda: be.topk(x, None, v, idx, (o, n, i), k, False), reps)
      bound_ms = 4.0 * o * n * i / HBM_BYTES_PER_S * 1e3
      res.update(ms=med, all_ms=all_ms, one_read_hbm_bound_ms=bound_ms, fraction_of_one_read_hbm_bound=bound_ms / med,
                 plan=list(backend.topk_plan(o, n, i, np.float32, k)))
    else:
      sv = torch.empty_like(x)
      si64 = torch.empty((o, n, i), dtype=torch.int64, device='cuda')
      v = torch.empty((o, k, i), dtype=torch.float32, device='cuda')
      idx = torch.empty((o, k, i), dtype=torch.int64, device='cuda')

      def parent():
        be.sort(x, sv, si64, (o, n, i))
        v.copy_(sv[:, :k])
        idx.copy_(si64[:, :k])
      med, all_ms = _time(parent, reps)
      res.update(ms=med, all_ms=all_ms, route='sort(values, indices) + slice')
  print(json.dumps(res), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--leg')
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--out')
  ap.add_argument('--limit', type=int, default=240, help='seconds per leg')
  a = ap.parse_args()
  if a.leg:
    run_leg(a.leg, a.reps)
    return 0
  lines = []
  for leg in LEGS:  # one child per leg; the parent never opens the GPU
    try:
      r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', leg, '--reps', str(a.reps)],
                         capture_output=True, text=True, timeout=max(a.limit, LIMIT_S.get(leg, 0)))
    except subprocess.TimeoutExpired:
      lines.append(json.dumps({'leg': leg, 'error': 'time limit'}))
      print(lines[-1], flush=True)
      break  # nothing more is started on the GPU after a leg that did not end
    out = [l for l in r.stdout.splitlines() if l.startswith('{')]
    if r.returncode != 0 or not out:
      lines.append(json.dumps({'leg': leg, 'error': 'exit %d' % r.returncode, 'stderr': r.stderr[-400:]}))
      print(lines[-1], flush=True)
      break
    lines.append(out[-1])
    print(out[-1], flush=True)
  got = {}
  for l in lines:
    d = json.loads(l)
    if 'ms' in d:
      got[d['leg']] = d['ms']
  summary = {'summary': True}
  for new, old in (('knn_fused', 'knn_parent'), ('topk_select', 'topk_sort')):
    for si in (0, 1):
      a_, b_ = got.get('%s:%d' % (new, si)), got.get('%s:%d' % (old, si))
      if a_ and b_:
        summary['%s:%d_speedup_over_parent_route' % (new, si)] = b_ / a_
  lines.append(json.dumps(summary))
  print(lines[-1], flush=True)
  if a.out:
    with open(a.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())
