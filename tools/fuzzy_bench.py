"""Measure spx_fuzzy_step on one GPU.

Legs: float32 and float64, N in {2^20, 2^22}, D = 128, K in {64, 256}, m = 2
(exponent 2), Gaussian points and centres built on the device from a seed:

  spx     HipBackend.fuzzy_step with labels, without U: the centre conversion,
          the fused kernel and the two reductions of the partials;

  torch   the composition a user of the parent commit, which has no fuzzy
          step, had, on the same GPU in the same run, chunked to 2^18 rows so
          that its (rows, K) intermediates fit: ``torch.cdist(x, c) ** 2 + eps``,
          ``d ** -e``, the row normalisation, ``argmin``, ``W.T @ x`` and
          ``W.sum(0)``, accumulated in float64.

Both are timed with HIP events after warm-up, in interleaved rounds in one
process (round r runs every leg once), and report the median and the minimum.
Before anything is timed the two routes are compared on the same input:
``agree`` is the share of equal labels, ``dsums`` the largest difference of the
sums relative to their largest magnitude.

``rate`` is the step's own operation count 4 N K D (2 N K D for the distances
as multiply-adds, 2 N K D for W^T X) over the spx median; ``of_peak`` divides it
by the vector / matrix peak of the dtype (157.3 TFLOP/s float32, 78.6 TFLOP/s
float64).  It is a whole-call rate, and the difference form spends three
operations where this count has two.

One child process per (dtype, N), each under ``timeout -k 10``, which signals
the child's whole process group; after a child that fails or runs past its
limit nothing more is started on the GPU: the table so far is written and the
tool exits 1.  Nothing here asserts a speed.

  python tools/fuzzy_bench.py --out profiles/fuzzy_bench.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1 << 20, 1 << 22)
KS = (64, 256)
D = 128
DTYPES = ('float32', 'float64')
PEAK = {'float32': 157.3e12, 'float64': 78.6e12}
CHUNK = 1 << 18
EPS = 1e-11
EXPONENT = 2.0  # m = 2


def data(n, k, dtype, seed=0):
  import torch
  g = torch.Generator(device='cuda')
  g.manual_seed(seed + n + k)
  X = torch.randn((n, D), generator=g, device='cuda', dtype=getattr(torch, dtype))
  C = torch.randn((k, D), generator=g, device='cuda', dtype=torch.float64)
  return X, C


def torch_step(X, C):
  """(labels, sums, counts) by the torch composition, CHUNK rows at a time."""
  import torch
  c = C.to(X.dtype)
  sums = torch.zeros(tuple(C.shape), dtype=torch.float64, device=X.device)
  counts = torch.zeros((C.shape[0],), dtype=torch.float64, device=X.device)
  labels = torch.empty((X.shape[0],), dtype=torch.int64, device=X.device)
  for r0 in range(0, X.shape[0], CHUNK):
    x = X[r0:r0 + CHUNK]
    d = torch.cdist(x, c) ** 2 + EPS
    labels[r0:r0 + CHUNK] = torch.argmin(d, dim=1)
    t = d ** -EXPONENT
    W = t / t.sum(dim=1, keepdim=True)
    sums += (W.t() @ x).to(torch.float64)
    counts += W.sum(dim=0).to(torch.float64)
  return labels, sums, counts


def child(dtype, n, rounds, warmup):
  """One (dtype, N): both K, both routes; one JSON line a K on stdout."""
  import torch
  import spartan_amd
  from spartan_amd import backend
  spartan_amd.initialize()
  be = backend.get()
  legs, rows = [], {}
  for k in KS:
    X, C = data(n, k, dtype)
    lab, _u, sums, counts = be.fuzzy_step(X, C, EXPONENT, EPS, 1.0, True, False)
    tl, ts, tc = torch_step(X, C)
    torch.cuda.synchronize()
    rows[k] = {'dtype': dtype, 'n': n, 'k': k, 'device': torch.cuda.get_device_name(0),
               'agree': float((lab == tl).double().mean().item()),
               'dsums': float(((sums - ts).abs().max() / ts.abs().max()).item())}
    legs.append((k, 'spx', (lambda X=X, C=C: be.fuzzy_step(X, C, EXPONENT, EPS, 1.0, True, False))))
    legs.append((k, 'torch', (lambda X=X, C=C: torch_step(X, C))))
  times = {i: [] for i in range(len(legs))}
  for r in range(warmup + rounds):
    for i, leg in enumerate(legs):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      leg[2]()
      b.record()
      b.synchronize()
      if r >= warmup:
        times[i].append(a.elapsed_time(b))
  for i, (k, which, _fn) in enumerate(legs):
    rows[k][which] = {'median': statistics.median(times[i]), 'min': min(times[i]), 'runs': len(times[i])}
  for k in KS:
    print('FUZZY_BENCH ' + json.dumps(rows[k]))


def run_child(dtype, n, args):
  """The child's rows, or a string saying why there are none."""
  cmd = ['timeout', '-k', '10', str(args.child_timeout), sys.executable, os.path.abspath(__file__), '--child', dtype,
         str(n), '--rounds', str(args.rounds), '--warmup', str(args.warmup)]
  with tempfile.TemporaryFile() as f:  # a file, not a pipe: nothing is held open by a killed child
    r = subprocess.run(cmd, stdin=subprocess.DEVNULL, stdout=f, stderr=subprocess.STDOUT)
    f.seek(0)
    text = f.read().decode(errors='replace')
  if r.returncode != 0:
    why = 'ran past %d s' % args.child_timeout if r.returncode in (124, 137) else 'exited %d' % r.returncode
    return 'child %s: %s' % (why, text[-300:])
  rows = [json.loads(line[len('FUZZY_BENCH '):]) for line in text.splitlines() if line.startswith('FUZZY_BENCH ')]
  return rows if len(rows) == len(KS) else 'child printed %d of %d rows: %s' % (len(rows), len(KS), text[-300:])


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fuzzy_bench.txt'))
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--sizes', type=int, nargs='*', default=list(SIZES))
  ap.add_argument('--child-timeout', type=int, default=240)
  ap.add_argument('--child', nargs=2, metavar=('DTYPE', 'N'), help='child mode: time one dtype and N and exit')
  args = ap.parse_args()
  if args.child:
    child(args.child[0], int(args.child[1]), args.rounds, args.warmup)
    return 0
  rows, failed, device = [], None, '?'
  todo = [(dtype, n) for dtype in DTYPES for n in args.sizes]
  for i, (dtype, n) in enumerate(todo):
    sys.stderr.write('fuzzy_bench: %s N=%d\n' % (dtype, n))
    got = run_child(dtype, n, args)
    if isinstance(got, str):
      failed = (dtype, n, got, todo[i + 1:])
      break  # nothing more is started on the GPU after a failure
    rows += got
    device = got[0]['device']
  lines = ['fuzzy_bench: %s, D = %d, m = 2, %d rounds after %d warm-up, HIP events; times in ms'
           % (device, D, args.rounds, args.warmup),
           'torch: cdist ** 2 + eps, d ** -e, row normalise, argmin, W.T @ x, in chunks of %d rows' % CHUNK, '',
           '%-8s %8s %4s %10s %10s %11s %10s %9s %8s %8s %9s' % ('dtype', 'N', 'K', 'spx med', 'spx min', 'torch med',
                                                              'torch/spx', 'TFLOP/s', 'of_peak', 'agree', 'dsums')]
  for row in rows:
    spx, tor = row['spx'], row['torch']
    rate = 4.0 * row['n'] * row['k'] * D / (spx['median'] * 1e-3)
    lines.append('%-8s %8d %4d %10.3f %10.3f %11.3f %10.2f %9.2f %7.1f%% %8.6f %9.2e'
                 % (row['dtype'], row['n'], row['k'], spx['median'], spx['min'], tor['median'],
                    tor['median'] / spx['median'], rate / 1e12, 100 * rate / PEAK[row['dtype']], row['agree'],
                    row['dsums']))
  if failed is not None:
    lines.append('%s N=%d: not measured: %s' % failed[:3])
    if failed[3]:
      lines.append('not started after that failure: %s' % ', '.join('%s N=%d' % t for t in failed[3]))
  text = '\n'.join(lines)
  print(text)
  with open(args.out, 'w') as f:
    f.write(text + '\n')
  return 0 if failed is None else 1


if __name__ == '__main__':
  sys.exit(main())
