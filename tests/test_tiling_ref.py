"""(f1) AutomaticTiling's solver pinned to the reference's OWN code: libspx's
spx_mincost_tiling against find_mincost_tiling compiled from
/root/reference/spartan/expr/tiling.cc:1-92 (oracle/build_ref.sh ->
oracle/_ref/libreftiling.so), on the AutomaticTiling graphs of the
configs[0] / configs[1] / configs[3] / configs[4] DAGs and on random graphs
with split pairs, repeated arcs and cost ties.  Identical chosen sets and
costs are required.

The reference's results for exactly these graphs are also recorded under
tests/golden/tiling_ref_*.npz (per graph: a CRC of the graph, the chosen set
as a bit mask, the cost), so the tests run wherever the repository is checked
out.  Where build() could compile the library (it needs the reference tree),
every graph is checked against the live library AND the live result against
the record; elsewhere against the record alone.  To record again, with the
library built:  SPARTAN_RECORD_TILING_REF=1 python -m pytest tests/test_tiling_ref.py"""
import os
import random
import zlib

import numpy as np
import pytest

from oracle import ref_tiling as RT
from oracle import tiling as OT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


class _Reference:
  """The reference solver's answers for one test's sequence of graphs."""

  def __init__(self, name):
    self.path = os.path.join(GOLDEN, 'tiling_ref_%s.npz' % name)
    self.record = os.environ.get('SPARTAN_RECORD_TILING_REF') == '1'
    self.live = RT.available()
    assert self.live or not self.record, 'recording needs oracle/_ref/libreftiling.so'
    self.rows = []
    self.i = 0
    if not self.record:
      with np.load(self.path) as z:
        self.crc, self.mask, self.cost = z['crc'], z['mask'], z['cost']

  def __call__(self, t, edges, pairs):
    crc = zlib.crc32(repr((int(t), [tuple(map(int, e)) for e in edges], [tuple(map(int, p)) for p in pairs])).encode())
    if self.record:
      chosen, cost = RT.mincost_tiling(t, edges, pairs)
      assert t <= 64
      self.rows.append((crc, sum(1 << u for u in chosen), cost))
      return chosen, cost
    i = self.i
    self.i += 1
    assert i < len(self.crc) and int(self.crc[i]) == crc, 'graph %d is not the recorded one: record again' % i
    want = [u for u in range(t) if (int(self.mask[i]) >> u) & 1], int(self.cost[i])
    if self.live:
      assert RT.mincost_tiling(t, edges, pairs) == want, (t, edges, pairs)
    return want

  def done(self):
    """Every recorded graph was asked for (or, recording, write the file)."""
    if self.record:
      crc, mask, cost = zip(*self.rows)
      np.savez_compressed(self.path, crc=np.array(crc, np.uint32), mask=np.array(mask, np.uint64),
                          cost=np.array(cost, np.int64))
    else:
      assert self.i == len(self.crc)


def _random_graphs(seed, count, tie_heavy=False):
  rnd = random.Random(seed)
  for _ in range(count):
    t = rnd.randint(2, 18)
    edges = []
    for v in range(1, t + 1):
      for _ in range(rnd.randint(1, 3)):
        c = rnd.choice([0, 0, 1, 1, 2]) if tie_heavy else rnd.choice([0, 0, 1, 5, 10, rnd.randint(0, 100)])
        edges.append((rnd.randint(0, v - 1), v, c))
    nodes = list(range(1, t))
    rnd.shuffle(nodes)
    pairs = [(nodes[i], nodes[i + 1]) for i in range(0, rnd.randint(0, len(nodes) // 2) * 2, 2)]
    yield t, edges, pairs


def test_random_graphs_match_reference():
  from spartan_amd import backend
  n = 0
  ref = _Reference('random')
  for t, edges, pairs in _random_graphs(11, 2000):
    want = ref(t, edges, pairs)
    assert backend.mincost_tiling(t, edges, pairs) == want, (t, edges, pairs)
    assert OT.mincost_tiling(t, edges, pairs) == want
    n += 1
  assert n == 2000
  ref.done()


def test_tie_heavy_graphs_match_reference():
  """Costs drawn from {0, 1, 2}: most split choices tie, which exercises the
  deferred-tie re-queue (tiling.cc:67-69) and its resolution."""
  from spartan_amd import backend
  ref = _Reference('ties')
  for t, edges, pairs in _random_graphs(12, 2000, tie_heavy=True):
    assert backend.mincost_tiling(t, edges, pairs) == ref(t, edges, pairs), (t, edges, pairs)
  ref.done()


def _captured_graphs(host_ctx, build):
  """Every (t, edges, split pairs) AutomaticTiling hands the solver while
  ``build()``'s expressions are optimised."""
  from spartan_amd import backend
  seen = []
  real = backend.mincost_tiling

  def spy(t, edges, pairs):
    seen.append((t, list(edges), list(pairs)))
    return real(t, edges, pairs)
  backend.mincost_tiling = spy
  try:
    build()
  finally:
    backend.mincost_tiling = real
  return seen


@pytest.mark.parametrize('W', [1, 3, 8])
def test_config_dags_match_reference(host_ctx, W):
  host_ctx(W)
  from spartan_amd import expr

  def build():
    # configs[0]: sum(dot(ones, ones)) (tests/benchmark_dot.py), configs[1]:
    # sum(x * y + exp(z), axis) on new arrays, configs[3]: dot of two new
    # arrays, configs[4]: the lreg gradient sum(x * (dot(x, w) - y), axis=0)
    n = 48
    expr.sum(expr.dot(expr.ones((n, n)), expr.ones((n, n)))).optimized()
    for ax in (0, 1, None):
      x, y, z = (expr.rand(n, 40, seed=s) for s in (1, 2, 3))
      expr.sum(x * y + expr.exp(z), axis=ax).optimized()
    expr.dot(expr.rand(n, 40, seed=4), expr.rand(40, 24, seed=5)).optimized()
    x = expr.rand(n, 8, seed=6)
    yv = expr.rand(n, 1, seed=7)
    w = np.full((8, 1), 0.5, np.float32)
    expr.sum(x * (expr.dot(x, w) - yv), axis=0).optimized()
  graphs = _captured_graphs(host_ctx, build)
  assert len(graphs) >= 6
  from spartan_amd import backend
  ref = _Reference('configs_w%d' % W)
  for t, edges, pairs in graphs:
    assert pairs, 'AutomaticTiling graphs carry split pairs'
    assert backend.mincost_tiling(t, edges, pairs) == ref(t, edges, pairs), (t, edges, pairs)
  ref.done()
