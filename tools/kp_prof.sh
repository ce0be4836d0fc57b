#!/bin/bash
# Dev build: k_kmeans_pp with per-wave s_memtime cycle counters per loop
# segment -> tools/bin/libspx_kpprof.so (read by tools/kp_prof.py).  The
# product source carries no instrumentation: this script inserts it into a
# copy of the sources at fixed code lines (it fails loudly if a line moved).
set -e
here=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$here/tools/bin"
python3 - "$here" <<'PY'
import sys
sys.path.insert(0, sys.argv[1] + '/tools')
from spx_variant import Variant
v = Variant('kpprof')
def ins(anchor, text, after=True):
    v.sub(anchor, anchor + text if after else text + anchor)
prof = '''
__device__ unsigned long long g_kp_prof[1024 * 8 * 8];
extern "C" int spx_dev_kp_prof(unsigned long long* host_out) {
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_kp_prof), sizeof(g_kp_prof)) == hipSuccess ? 0 : 1;
}
#define KPT(k) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); pacc_[k] += now_ - plast_; plast_ = now_; }
'''
ins('template <int KS, int NCT>\nstruct KpStep {', prof, after=False)
ins('  const int col0 = CPW * s + CPL * hr;\n',
    '  unsigned long long pacc_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, plast_ = __builtin_amdgcn_s_memtime();\n')
v.sub('    __syncthreads();\n    if constexpr (c == 0)\n', '    KPT(7)\n    __syncthreads();\n    KPT(0)\n    if constexpr (c == 0)\n')
ins('    ks_unroll(mk, std::make_integer_sequence<int, KS>{});\n', '    KPT(1)\n')  # after the woven chain
ins('    // labels (-1 for an undecided row', '    KPT(2)\n', after=False)
ins('    load(r, tt + KP_AHEAD);\n', '    KPT(3)\n')
if v.count('    // (4) each decided row'):  # decision in the vector role (round-4 v3 / v4)
    ins('    // (4) each decided row', '    KPT(4)\n', after=False)
    ins('    // (6) stage of unit t + 1\n', '    KPT(5)\n', after=False)
    ins('    if (s == 0 && h == 0) dres[', '    KPT(6)\n', after=False)
else:  # decision in the matrix role: vector = fold + exv (4), stage (6)
    ins('    __builtin_amdgcn_sched_barrier(0);\n    if (us < nit) {\n', '    KPT(4)\n', after=False)
    ins('      stage(rs, mu4, us);\n    }\n', '    KPT(6)\n')
v.sub('  if (t < K) pcnt[(i64)bk * K + t] = cnts[t];\n}\n\ntemplate <int KS, int NCT>\nstatic void kp_launch',
              '  if (t < K) pcnt[(i64)bk * K + t] = cnts[t];\n  if (lane == 0 && KS == 8 && NCT == 8)\n'
              '    for (int k = 0; k < 8; ++k) g_kp_prof[(blockIdx.x * 8 + w) * 8 + k] = pacc_[k];\n}\n\n'
              'template <int KS, int NCT>\nstatic void kp_launch')
v.build()
PY
