"""Measure spx_csrmm on one GPU.

float32, p = 1 (SpMV) and p = 16, three matrices:

  pagerank  examples/pagerank.site_graph(2^22 pages, 10 out-links, 0.9): the
            reference's PageRank benchmark shape for one worker;
  uniform   2^22 rows x 32 nonzeros, random columns in 2^22;
  skew      the same 2^27 nonzeros, half of them in one row, the rest in rows
            of 32 alternating with empty rows.

Each leg is timed by HIP events around single calls after warm-up, ours and the
vendor route (``torch.sparse_csr_tensor @ dense`` on the same arrays, int32
indices) alternating in one process; median and minimum over the rounds.  Ours
runs with a prepared workspace (the analysis is made by the warm-up calls).
``fraction`` is the time to move the bytes of the model

    nnz (4 + itemsize) + 8 (m + 1) + (n p + m p) itemsize

at 8 TB/s over the median time.  Before anything is timed, column 0 of both
routes' results is compared with a float64 result (``err / u``: the largest
error over 1.5 x the row's absolute sum, in units of u = 2^-24, ours and the
vendor's).  A vendor call that takes longer than --slow-ms is timed once, not
every round.  Nothing here asserts a speed.

  python tools/sparse_bench.py --out profiles/sparse_bench.txt
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def _events(fn, torch):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sparse_bench.txt'))
  ap.add_argument('--log2-rows', type=int, default=22)
  ap.add_argument('--rounds', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--slow-ms', type=float, default=500.0, help='a vendor call slower than this is timed once')
  ap.add_argument('--matrices', nargs='*', default=['pagerank', 'uniform', 'skew'])
  args = ap.parse_args()
  import numpy as np
  import torch
  import spartan_amd
  from spartan_amd import backend
  from spartan_amd.examples.pagerank import site_graph
  spartan_amd.initialize()
  be = backend.get()
  dev = torch.device('cuda', torch.cuda.current_device())
  m = n = 2 ** args.log2_rows
  per_row = 32

  def pagerank():
    S = site_graph(n, 10, 0.9, seed=1, tile_hint=(n, n)).force()
    (t,) = S.local.values()
    return t.rowptr, t.col, t.val

  def uniform():
    g = torch.Generator(device=dev).manual_seed(2)
    col = torch.randint(0, n, (m, per_row), dtype=torch.int32, device=dev, generator=g).sort(dim=1).values
    val = torch.rand(m * per_row, dtype=torch.float32, device=dev, generator=g) + 0.5
    rowptr = torch.arange(0, m + 1, dtype=torch.int64, device=dev) * per_row
    return rowptr, col.reshape(-1).contiguous(), val

  def skew():
    g = torch.Generator(device=dev).manual_seed(3)
    half = m * per_row // 2
    big = m // 2  # an even row: the odd rows hold 32 each
    lens = torch.zeros(m, dtype=torch.int64, device=dev)
    lens[1::2] = per_row
    lens[big] = half
    rowptr = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(lens, 0)
    short = torch.randint(0, n, (m // 2, per_row), dtype=torch.int32, device=dev, generator=g).sort(dim=1).values
    long_cols = torch.arange(0, n, dtype=torch.int32, device=dev).repeat_interleave(half // n)
    first = short[:big // 2].reshape(-1)
    col = torch.cat([first, long_cols, short[big // 2:].reshape(-1)]).contiguous()
    val = torch.rand(col.numel(), dtype=torch.float32, device=dev, generator=g) + 0.5
    assert int(rowptr[-1]) == col.numel() == m * per_row
    return rowptr, col, val

  lines = ['device %s, float32, %d rounds after %d warm-up calls, HIP events per call'
           % (torch.cuda.get_device_name(dev), args.rounds, args.warmup),
           '%-9s %3s %12s %9s %9s %9s %9s %9s %7s %9s %9s' % ('matrix', 'p', 'nnz', 'model MB', 'ours ms', 'ours min',
                                                             'fraction', 'vendor ms', 'ratio', 'err / u', 'vendor')]
  rows = []
  for name, make in (('pagerank', pagerank), ('uniform', uniform), ('skew', skew)):
    if name not in args.matrices:
      continue
    rowptr, col, val = make()
    nnz = int(col.numel())
    vendor_err = None
    try:
      A = torch.sparse_csr_tensor(rowptr.to(torch.int32), col, val, size=(m, n))
    except Exception as e:  # pragma: no cover - depends on the installed torch
      A, vendor_err = None, repr(e)[:200]
    # per-row sums of |val| from one running sum (an index_add_ here would be 2^26 float64 atomics on one address
    # for the skew matrix's long row)
    run = torch.zeros(nnz + 1, dtype=torch.float64, device=dev)
    torch.cumsum(val.abs().double(), 0, out=run[1:])
    absrow = run[rowptr[1:]] - run[rowptr[:-1]]
    del run
    print('%s: built, nnz %d' % (name, nnz), flush=True)
    for p in (1, 16):
      B = torch.rand((n, p), dtype=torch.float32, device=dev) + 0.5
      C = torch.empty((m, p), dtype=torch.float32, device=dev)
      ws = backend.CsrWorkspace()
      g, T, rpb = backend.csrmm_plan(np.float32, m, nnz, p)

      def ours():
        be.csrmm(rowptr, col, val, n, B, C, 1.0, 0.0, 0, ws)

      def vendor():
        return A @ B

      legs = {'ours': ours}
      diff = None
      rounds = {'ours': args.rounds}
      print('%s p=%d: ours first call %.3f ms' % (name, p, _events(ours, torch)), flush=True)
      if A is not None:
        try:
          t0 = time.time()
          V = vendor()
          torch.cuda.synchronize()
          first = (time.time() - t0) * 1e3
          print('%s p=%d: vendor first call %.1f ms' % (name, p, first), flush=True)
          rounds['vendor'] = args.rounds if first < args.slow_ms else 0
          # column 0 of both against a float64 result (running sum of the products, differenced at the row ends);
          # B <= 1.5: |A| |B| <= 1.5 absrow
          run = torch.zeros(nnz + 1, dtype=torch.float64, device=dev)
          torch.cumsum(val.double() * B[:, 0][col.long()].double(), 0, out=run[1:])
          ref = run[rowptr[1:]] - run[rowptr[:-1]]
          del run
          scale = (1.5 * absrow).clamp_min(1e-300) * 2.0 ** -24
          diff = (float(((C[:, 0].double() - ref).abs() / scale).max()), float(((V[:, 0].double() - ref).abs() / scale).max()))
          del ref, scale
          legs['vendor'] = vendor
          del V
        except Exception as e:  # pragma: no cover
          vendor_err = repr(e)[:200]
      if rounds.get('vendor') == 0:  # too slow to repeat: one more call, timed
        ms_slow = [_events(vendor, torch)]
        del legs['vendor']
      for _ in range(args.warmup):
        for fn in legs.values():
          fn()
      torch.cuda.synchronize()
      ms = {k: [] for k in legs}
      for _ in range(args.rounds):
        for k, fn in legs.items():
          ms[k].append(_events(fn, torch))
      if rounds.get('vendor') == 0:
        ms['vendor'] = ms_slow
      model = nnz * (4 + 4) + 8 * (m + 1) + (n * p + m * p) * 4
      ideal = model / HBM_BYTES_PER_S * 1e3
      o_med, o_min = statistics.median(ms['ours']), min(ms['ours'])
      row = {'matrix': name, 'p': p, 'm': m, 'n': n, 'nnz': nnz, 'g': g, 'T': T, 'model_bytes': model,
             'ours_ms_median': round(o_med, 4), 'ours_ms_min': round(o_min, 4), 'fraction_of_8TBs': round(ideal / o_med, 4)}
      v_med = None
      if 'vendor' in ms:
        v_med = statistics.median(ms['vendor'])
        row.update(vendor_ms_median=round(v_med, 4), vendor_ms_min=round(min(ms['vendor']), 4),
                   ours_over_vendor=round(o_med / v_med, 3), err_ours_u=round(diff[0], 3), err_vendor_u=round(diff[1], 3))
      else:
        row['vendor_error'] = vendor_err
      rows.append(row)
      lines.append('%-9s %3d %12d %9.1f %9.3f %9.3f %9.3f %9s %7s %9s %9s'
                   % (name, p, nnz, model / 1e6, o_med, o_min, ideal / o_med,
                      '%.3f' % v_med if v_med else 'n/a', '%.2f' % (o_med / v_med) if v_med else 'n/a',
                      '%.3g' % diff[0] if diff is not None else 'n/a', '%.3g' % diff[1] if diff is not None else 'n/a'))
      print(lines[-1], flush=True)
      del B, C
    del A, rowptr, col, val, absrow
    torch.cuda.empty_cache()
  lines.append('ratio = ours / vendor (median times; below 1: ours is faster).  One box, one sitting: the HBM rate of '
               'these boxes differs by several per cent box to box, the ratio is the same-box figure.')
  lines.append(json.dumps({'rows': rows}))
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
  print('\n'.join(lines[:2]))


if __name__ == '__main__':
  main()
