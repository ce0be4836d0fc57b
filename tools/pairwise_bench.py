"""Measure spx_pairwise on one GPU.

Legs: float32 and float64, n = m in {8192, 32768} points of d in {16, 128}
standard-normal features (Y = X), built on the device from a seed:

  out     HipBackend.pairwise with ``out`` only: the materialising call;
  deg     the degree pass: rbf, ``row_sums`` only, nothing stored;
  full    ``expr.normalized_affinity`` forced: the degree pass, the n-element
          1 / sqrt(D) in torch, the scaled pass that stores L;

  parent  what a user of the parent commit, which has no pair kernel, had, on
          the same GPU in the same run: the broadcast expression
          ``sum(square(X[:, None, :] - Y[None, :, :]), axis=2)`` of
          ``KMeans._fit_broadcast`` (route ``expr``; ``out`` is then timed with
          'sqeuclidean').  Where the expression does not run, or its
          n * m * d iteration space is above ``--expr-max`` elements (2^40: a
          guard, above every default shape), ``torch.cdist`` stands in (route
          ``cdist``, and ``out`` is then timed with 'euclidean');

  cdist   ``torch.cdist(X, X)`` at every shape, beside the parent route: the
          euclidean distance by the Gram form |x|^2 + |y|^2 - 2 x.y on the
          matrix cores, which has neither the exact zeros nor the bitwise
          symmetry of the difference form;

  model   the kernel's own operation model: 2 n m d lane-operations (one
          subtraction, one fused multiply-add per pair and feature) at the
          vector issue rate, 256 CUs x 4 SIMDs x 32 lanes a cycle at 2.4 GHz =
          7.86e13 / s in float32 and half that in float64.  ``of_issue`` is
          model / out; for ``full`` the model is two passes.

All are timed with HIP events after warm-up, in interleaved rounds in one
process (round r runs every leg once), and report the median; a parent leg
whose first run takes more than 0.5 s is timed over three rounds only.  Before
anything is timed the two routes are compared on the same input: ``diff`` is
the largest |out - parent| over the largest |parent|.

``--lib PATH`` times another build of the library.

One child process per dtype, under ``timeout -k 10``, which signals the
child's whole process group; after a child that fails or runs past its limit
nothing more is started on the GPU: the table so far is written and the tool
exits 1.  Nothing here asserts a speed.

  python tools/pairwise_bench.py --out profiles/pairwise_bench.txt
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

SIZES = (8192, 32768)
DIMS = (16, 128)
DTYPES = ('float32', 'float64')
ISSUE = {'float32': 256 * 4 * 32 * 2.4e9, 'float64': 256 * 4 * 16 * 2.4e9}  # lane-operations / s
SLOW_MS = 500.0


def data(n, d, dtype, seed=0):
  import torch
  g = torch.Generator(device='cuda')
  g.manual_seed(seed + n + d)
  return torch.randn((n, d), generator=g, device='cuda', dtype=getattr(torch, dtype))


def child(dtype, sizes, dims, rounds, warmup, expr_max, lib):
  """One dtype: every shape, every leg; one JSON line a shape on stdout."""
  import torch
  import spartan_amd
  from spartan_amd import backend, binding, expr
  from spartan_amd.array import distarray, extent
  if lib:
    binding.load_library(lib)
  spartan_amd.initialize()
  be = backend.get()

  def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)

  legs, rows = [], {}
  for n in sizes:
    for d in dims:
      X = data(n, d, dtype)
      gamma = 0.5 / d
      xe = expr.lazify(expr.from_numpy(X.cpu().numpy()).force())

      def parent_expr(xe=xe, n=n, d=d):
        a, b = expr.reshape(xe, (n, 1, d)), expr.reshape(xe, (1, n, d))
        return distarray.as_array(expr.sum(expr.square(a - b), axis=2).optimized().force())

      route, why = 'expr', ''
      if float(n) * n * d > expr_max:
        route, why = 'cdist', 'iteration space above --expr-max'
      else:
        try:
          ref = parent_expr()
          ref = ref.fetch(extent.from_shape(ref.shape)).reshape(n, n)  # (one worker: the device block itself)
        except Exception as e:  # the expression does not run at this shape
          route, why = 'cdist', '%s: %s' % (type(e).__name__, str(e)[:80])
      metric = 'sqeuclidean' if route == 'expr' else 'euclidean'
      got = be.pairwise(X, X, metric, gamma, out=True)[0]
      if route == 'expr':
        parent = parent_expr
      else:
        parent = (lambda X=X: torch.cdist(X, X))
        ref = parent()
      torch.cuda.synchronize()
      diff = float(((got - ref).abs().max() / ref.abs().max()).item())
      del got, ref
      key = (n, d)
      rows[key] = {'dtype': dtype, 'n': n, 'd': d, 'device': torch.cuda.get_device_name(0), 'route': route,
                   'why': why, 'diff': diff, 'splits': binding.pairwise_plan(dtype, n, n)[2]}
      first = timed(parent)  # (also the parent leg's warm-up)
      rows[key]['parent_rounds'] = rounds if first <= SLOW_MS else min(rounds, 3)

      def full(xe=xe, gamma=gamma):
        L, _D = expr.normalized_affinity(xe, metric='rbf', gamma=gamma)
        return L.force()

      legs.append((key, 'out', (lambda X=X, metric=metric, gamma=gamma: be.pairwise(X, X, metric, gamma, out=True))))
      legs.append((key, 'deg', (lambda X=X, gamma=gamma: be.pairwise(X, X, 'rbf', gamma, row_sums=True))))
      legs.append((key, 'full', full))
      legs.append((key, 'parent', parent))
      legs.append((key, 'cdist', (lambda X=X: torch.cdist(X, X))))
  times = {i: [] for i in range(len(legs))}
  for r in range(warmup + rounds):
    for i, (key, which, fn) in enumerate(legs):
      if which == 'parent' and r >= warmup + rows[key]['parent_rounds']:
        continue
      t = timed(fn)
      if r >= warmup:
        times[i].append(t)
  for i, (key, which, _fn) in enumerate(legs):
    rows[key][which] = {'median': statistics.median(times[i]), 'min': min(times[i]), 'runs': len(times[i])}
  for key in rows:
    print('PAIRWISE_BENCH ' + json.dumps(rows[key]))


def run_child(dtype, args):
  """The child's rows, or a string saying why there are none."""
  cmd = (['timeout', '-k', '10', str(args.child_timeout), sys.executable, os.path.abspath(__file__), '--child', dtype,
          '--rounds', str(args.rounds), '--warmup', str(args.warmup), '--expr-max', str(args.expr_max), '--sizes']
         + [str(n) for n in args.sizes] + ['--dims'] + [str(d) for d in args.dims])
  if args.lib:
    cmd += ['--lib', args.lib]
  with tempfile.TemporaryFile() as f:  # a file, not a pipe: nothing is held open by a killed child
    r = subprocess.run(cmd, stdin=subprocess.DEVNULL, stdout=f, stderr=subprocess.STDOUT)
    f.seek(0)
    text = f.read().decode(errors='replace')
  if r.returncode != 0:
    why = 'ran past %d s' % args.child_timeout if r.returncode in (124, 137) else 'exited %d' % r.returncode
    return 'child %s: %s' % (why, text[-300:])
  rows = [json.loads(line[len('PAIRWISE_BENCH '):]) for line in text.splitlines()
          if line.startswith('PAIRWISE_BENCH ')]
  want = len(args.sizes) * len(args.dims)
  return rows if len(rows) == want else 'child printed %d of %d rows: %s' % (len(rows), want, text[-300:])


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pairwise_bench.txt'))
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--sizes', type=int, nargs='*', default=list(SIZES))
  ap.add_argument('--dims', type=int, nargs='*', default=list(DIMS))
  ap.add_argument('--expr-max', type=float, default=float(2 ** 40))
  ap.add_argument('--lib', default=None, help='another build of libspx.so to time')
  ap.add_argument('--child-timeout', type=int, default=400)
  ap.add_argument('--child', metavar='DTYPE', help='child mode: time one dtype and exit')
  args = ap.parse_args()
  if args.child:
    child(args.child, args.sizes, args.dims, args.rounds, args.warmup, args.expr_max, args.lib)
    return 0
  rows, failed, device = [], None, '?'
  for i, dtype in enumerate(DTYPES):
    sys.stderr.write('pairwise_bench: %s\n' % dtype)
    got = run_child(dtype, args)
    if isinstance(got, str):
      failed = (dtype, got, DTYPES[i + 1:])
      break  # nothing more is started on the GPU after a failure
    rows += got
    device = got[0]['device']
  lines = ['pairwise_bench: %s, n = m, Y = X, %d rounds after %d warm-up, HIP events; medians in ms%s'
           % (device, args.rounds, args.warmup, '; library %s' % os.path.basename(args.lib) if args.lib else ''),
           'out: spx_pairwise, out only (sqeuclidean beside expr, euclidean beside cdist); deg: rbf row sums only; '
           'full: expr.normalized_affinity',
           'parent: route expr = sum(square(X[:, None, :] - Y[None, :, :]), axis=2); route cdist = torch.cdist; '
           'cdist: torch.cdist (euclidean, Gram form on the matrix cores)',
           'model: 2 n m d lane-operations at 7.86e13 / s (float32), 3.93e13 / s (float64); of_issue = model / out',
           '',
           '%-8s %6s %4s %6s %9s %9s %9s %6s %10s %10s %9s %9s %8s %9s'
           % ('dtype', 'n', 'd', 'splits', 'out', 'deg', 'full', 'route', 'parent', 'parent/out', 'cdist', 'model',
              'of_issue', 'diff')]
  notes = []
  for row in rows:
    model = 2.0 * row['n'] * row['n'] * row['d'] / ISSUE[row['dtype']] * 1e3
    out, deg, full, par, cd = (row[k]['median'] for k in ('out', 'deg', 'full', 'parent', 'cdist'))
    lines.append('%-8s %6d %4d %6d %9.3f %9.3f %9.3f %6s %10.3f %10.2f %9.3f %9.3f %7.1f%% %9.2e'
                 % (row['dtype'], row['n'], row['d'], row['splits'], out, deg, full, row['route'], par, par / out, cd,
                    model, 100 * model / out, row['diff']))
    if row['why']:
      notes.append('%s n %d d %d: cdist because: %s' % (row['dtype'], row['n'], row['d'], row['why']))
    if row['parent']['runs'] < args.rounds:
      notes.append('%s n %d d %d: parent over %d rounds' % (row['dtype'], row['n'], row['d'], row['parent']['runs']))
  lines += [''] + notes if notes else []
  if failed is not None:
    lines.append('%s: not measured: %s' % failed[:2])
    if failed[2]:
      lines.append('not started after that failure: %s' % ', '.join(failed[2]))
  text = '\n'.join(lines)
  print(text)
  with open(args.out, 'w') as f:
    f.write(text + '\n')
  return 0 if failed is None else 1


if __name__ == '__main__':
  sys.exit(main())
