"""Measure spx_apsp on one GPU.

Legs, float32 and float64, n in {2048, 4096, 8192}, a random integer-weight
digraph (about 3.5 edges a row, weights 1 .. 49: every path sum is exact):

  spx     HipBackend.apsp: init, then per pivot block the diagonal, panel and
          rest launches (3 ceil(n / b) + 1 launches on one stream).

Beside each leg, from the same run:

  torch   the route a user of the parent commit, which has no shortest-path
          node, had: n dependent passes of
          ``D = torch.minimum(D, D[:, k:k+1] + D[k:k+1, :])`` on the same GPU.
          A loop that takes more than --slow-ms is timed once, not every round.

GPU legs are timed with HIP events after warm-up, in interleaved rounds in one
process (round r runs every leg once), and report the median and the minimum.
Before anything is timed the two routes are compared on the same input: on
integer weights they must agree bit for bit (``check``).

Rates: the recurrence needs 2 n^3 operations (n^3 additions, n^3 minima).
``rate`` is 2 n^3 over the spx median; ``of_peak`` divides it by the VALU rate
of one simple operation per lane and clock -- 256 CUs x 4 SIMDs x 32 lanes x
2.4 GHz = 78.6e12 / s for float32 (half the 157.3 TFLOP/s vector peak, which
counts a fused multiply-add as two), and half of that for float64.  It is a
whole-call rate: the cheap phases and the launch gaps are inside it.

Per-phase kernel times come from a run of its own: for every n the tool starts
``rocprofv3 --kernel-trace --stats`` on a child process that runs both dtypes
(``--trace-n``), and reads the child's kernel statistics.  ``share`` is each
kernel's part of the summed kernel time; ``model`` is its part of the 2 n^3
operations (diag 1 / nb^2, panel 2 (nb - 1) / nb^2, rest (nb - 1)^2 / nb^2).
The child runs under ``timeout -k 10``; after a child that fails or runs past
its limit nothing more is started on the GPU: the table so far is written and
the tool exits 1.  --no-trace skips the traces.  Nothing here asserts a speed.

Prints the table and writes it to --out.

  python tools/apsp_bench.py --out profiles/apsp_bench.txt
"""
import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (2048, 4096, 8192)
DTYPES = ('float32', 'float64')
LANE_OPS = {'float32': 256 * 4 * 32 * 2.4e9, 'float64': 256 * 4 * 32 * 2.4e9 / 2}
PHASES = ('k_apsp_init', 'k_apsp_diag', 'k_apsp_panel', 'k_apsp_rest', 'k_apsp_fill')


def graph(n, dtype, seed=0):
  """The 'int' kind of tests/graph_ref.py at bench size, built on the device."""
  import torch
  g = torch.Generator(device='cuda')
  g.manual_seed(seed + n)
  mask = torch.rand((n, n), generator=g, device='cuda') < 3.5 / n
  w = torch.randint(1, 50, (n, n), generator=g, device='cuda')
  G = torch.where(mask, w, torch.zeros_like(w)).to(getattr(torch, dtype))
  G.fill_diagonal_(0)
  return G


def torch_loop(G):
  """n dependent passes over the n x n matrix: what can be written without spx_apsp."""
  import torch
  D = torch.where(G > 0, G, torch.full_like(G, float('inf')))
  D.fill_diagonal_(0)
  for k in range(D.shape[0]):
    D = torch.minimum(D, D[:, k:k + 1] + D[k:k + 1, :])
  return D


def _summary(ms):
  return {'median': statistics.median(ms), 'min': min(ms), 'runs': len(ms)}


def trace_child(n):
  """Under rocprofv3: both dtypes at one n, one warm-up call and two more."""
  import torch
  import spartan_amd
  from spartan_amd import backend
  spartan_amd.initialize()
  be = backend.get()
  for dtype in DTYPES:
    G = graph(n, dtype)
    for _ in range(3):
      be.apsp(G)
    torch.cuda.synchronize()


def trace(n, timeout):
  """{dtype: {kernel: total ns over the child's calls}} from a rocprofv3 child, or a string saying why not."""
  exe = shutil.which('rocprofv3') or os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'bin', 'rocprofv3')
  if not os.path.exists(exe):
    return 'rocprofv3 not found'
  d = tempfile.mkdtemp(prefix='apsp_trace_')
  try:
    # `timeout` puts rocprofv3 and the python below it into one process group
    # and signals the whole group, so a child past its limit leaves nothing on
    # the GPU; the output goes to a file, so no pipe is held open either
    cmd = ['timeout', '-k', '10', str(timeout), exe, '--kernel-trace', '--stats', '-d', d, '-o', 't',
           '--output-format', 'csv', '--', sys.executable, os.path.abspath(__file__), '--trace-n', str(n)]
    log = os.path.join(d, 'child.log')
    with open(log, 'wb') as f:
      r = subprocess.run(cmd, stdin=subprocess.DEVNULL, stdout=f, stderr=subprocess.STDOUT)
    if r.returncode != 0:
      with open(log, 'rb') as f:
        tail = f.read()[-300:].decode(errors='replace')
      why = 'ran past %d s' % timeout if r.returncode in (124, 137) else 'exited %d' % r.returncode
      return 'rocprofv3 child %s: %s' % (why, tail)
    files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
      return 'no kernel_stats.csv written'
    out = {dt: {} for dt in DTYPES}
    with open(files[0]) as f:
      for row in csv.DictReader(f):
        name = row['Name']
        for ph in PHASES:
          if ph + '<' in name:
            dt = 'float64' if ph + '<double>' in name else 'float32'
            out[dt][ph] = out[dt].get(ph, 0) + int(row['TotalDurationNs'])
    return out
  finally:
    shutil.rmtree(d, ignore_errors=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'apsp_bench.txt'))
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--slow-ms', type=float, default=300.0)
  ap.add_argument('--sizes', type=int, nargs='*', default=list(SIZES))
  ap.add_argument('--no-trace', action='store_true')
  ap.add_argument('--trace-timeout', type=int, default=240)
  ap.add_argument('--trace-n', type=int, default=0, help='child mode: run spx_apsp at this n and exit')
  args = ap.parse_args()
  if args.trace_n:
    trace_child(args.trace_n)
    return
  import numpy as np
  import torch
  import spartan_amd
  from spartan_amd import backend
  spartan_amd.initialize()
  be = backend.get()
  dev = torch.device('cuda', torch.cuda.current_device())
  rows, legs = {}, []
  for dtype in DTYPES:
    for n in args.sizes:
      key = (dtype, n)
      G = graph(n, dtype)
      D, info = be.apsp(G)
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      T = torch_loop(G)
      torch.cuda.synchronize()
      once = (time.perf_counter() - t0) * 1e3
      row = rows[key] = {'info': int(info.item()), 'check': bool(torch.equal(D, T)),
                         'unreachable': float(torch.isinf(D).float().mean().item())}
      del D, T
      legs.append((key, 'spx', (lambda G=G: be.apsp(G))))
      if once > args.slow_ms:
        row['torch'] = dict(_summary([once]), note='one host-timed loop')
      else:
        legs.append((key, 'torch', (lambda G=G: torch_loop(G))))
      sys.stderr.write('apsp_bench: %s n=%d set up (torch loop %.0f ms)\n' % (dtype, n, once))
  times = {i: [] for i in range(len(legs))}
  for r in range(args.warmup + args.rounds):
    for i, leg in enumerate(legs):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      leg[2]()
      b.record()
      b.synchronize()
      if r >= args.warmup:
        times[i].append(a.elapsed_time(b))
  for i, (key, which, _fn) in enumerate(legs):
    rows[key][which] = _summary(times[i])
  del legs
  torch.cuda.empty_cache()
  name = torch.cuda.get_device_name(dev)
  traces, failed = {}, None
  if not args.no_trace:
    for n in args.sizes:
      sys.stderr.write('apsp_bench: kernel trace at n=%d\n' % n)
      traces[n] = trace(n, args.trace_timeout)
      if isinstance(traces[n], str):
        failed = n
        break  # nothing more is started on the GPU after a failure
  lines = ['apsp_bench: %s, %d rounds after %d warm-up, HIP events; times in ms' % (name, args.rounds, args.warmup),
           'tile b: float32 %d, float64 %d' % (backend.apsp_plan(np.float32), backend.apsp_plan(np.float64)), '',
           '%-8s %6s %10s %10s %12s %10s %9s %8s %6s %s' % ('dtype', 'n', 'spx med', 'spx min', 'torch med',
                                                          'torch/spx', 'Gop/s', 'of_peak', 'equal', 'unreachable')]
  for (dtype, n), row in rows.items():
    spx, tor = row['spx'], row['torch']
    rate = 2.0 * n ** 3 / (spx['median'] * 1e-3)
    lines.append('%-8s %6d %10.3f %10.3f %12.1f %10.1f %9.0f %7.1f%% %6s %10.3f%s'
                 % (dtype, n, spx['median'], spx['min'], tor['median'], tor['median'] / spx['median'], rate / 1e9,
                    100 * rate / LANE_OPS[dtype], row['check'] and row['info'] == 0, row['unreachable'],
                    '  (torch: %s)' % tor['note'] if 'note' in tor else ''))
  if traces:
    lines += ['', 'kernel time per phase (rocprofv3 --kernel-trace --stats, a run of its own; 3 calls summed)',
              '%-8s %6s %-13s %12s %8s %8s' % ('dtype', 'n', 'kernel', 'ms per call', 'share', 'model')]
    for n, tr in traces.items():
      if isinstance(tr, str):
        skipped = [m for m in args.sizes if m not in traces]
        lines.append('n=%d: not measured: %s' % (n, tr))
        if skipped:
          lines.append('n=%s: not started after that failure' % ', '.join(str(m) for m in skipped))
        continue
      b = backend.apsp_plan(np.float32)
      nb = -(-n // b)
      model = {'k_apsp_diag': 1.0 / nb ** 2, 'k_apsp_panel': 2.0 * (nb - 1) / nb ** 2,
               'k_apsp_rest': float(nb - 1) ** 2 / nb ** 2}
      for dtype in DTYPES:
        total = sum(tr[dtype].values()) or 1
        for ph in PHASES:
          if ph in tr[dtype]:
            lines.append('%-8s %6d %-13s %12.3f %7.1f%% %7.1f%%' % (dtype, n, ph, tr[dtype][ph] / 3e6,
                                                                  100.0 * tr[dtype][ph] / total,
                                                                  100.0 * model.get(ph, 0.0)))
        lines.append('%-8s %6d %-13s %12.3f' % (dtype, n, 'all kernels', total / 3e6))
  text = '\n'.join(lines)
  print(text)
  with open(args.out, 'w') as f:
    f.write(text + '\n')
  return 0 if failed is None else 1


if __name__ == '__main__':
  sys.exit(main())
