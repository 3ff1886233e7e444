// cic2.hip -- ac_cic_dec_full at the rates it is deployed at (R = 32 ... 256): two stages in one launch.
//
// The factorisation R = R1 R2, the two stages and the kernel itself are in cic2_kernels.hpp, with the table of compiled stage-1 shapes.
// This unit holds the host side (cic2_factor, cic2_hist_len, launch_cic2) and compiles the first shape; cic2_b.hip .. cic2_f.hip compile
// the others and cic2_s8.hip .. cic2_s8_c.hip the byte-row shapes (ACDSP_FLAG_IN_BYTES), for compile time.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cic2_kernels.hpp"

namespace acdsp {

ACDSP_CIC2_COMPILE(s16_r16)

namespace {

// compiled shapes: (container bytes, R1) -> digit planes / K blocks compiled in, steps per load group
struct Shape { int in_eb, R1, pct, nbt, m; hipError_t (*launch)(int, int, dim3, hipStream_t, const Cic2Args &, const v4i *); };
#define ACDSP_CIC2_ROW(TIN, TAG, EB, R1V, PCTV, NBTV) {EB, R1V, PCTV, NBTV, ((R1V) * (EB)) % 4 == 0 ? 1 : 2, cic2_launch_##TAG},
const Shape kShapes[] = {ACDSP_CIC2_SHAPES(ACDSP_CIC2_ROW)};
#undef ACDSP_CIC2_ROW

const Shape *find_shape(int in_eb, int R1) {
  for (const Shape &s : kShapes) { if (s.in_eb == in_eb && s.R1 == R1) { return &s; } }
  return nullptr;
}

}  // namespace

// Which factorisation R = R1 R2 (R1 a compiled stage-1 rate of this container width) serves the parameter set; false: none.
bool cic2_factor(int in_eb, int R, int me, int N, int *R1_out, int *R2_out, int *wu_out) {
  if (N < 1 || N > kCic2MaxN || N * me > kCic2Zero) { return false; }
  static const char *force = getenv("ACDSP_CIC2_R1");   // A/B knob: the stage-1 rate to use where it divides R
  for (const Shape &s : kShapes) {
    if (s.in_eb != in_eb || R % s.R1 != 0 || R / s.R1 < 2) { continue; }
    if (force && atoi(force) != s.R1) { continue; }
    const int R2 = R / s.R1;
    const int wu = (N * (R2 * me - 1) + 255) / 256;
    if (wu < 1 || wu > 2) { continue; }
    // the stage-1 taps of this rate must fit the digit planes / K blocks the shape was compiled with, at both extreme phases of a call start
    // (R1 = 15 at N = 6 needs a third plane: R = 45 then goes to R1 = 5, not to the recurrence kernel)
    std::vector<int64_t> taps;
    cic2_stage1_taps(s.R1, N, &taps);
    bool fits = true;
    for (int ph : {0, 15}) {
      FirGenPlan probe;
      std::vector<uint32_t> fr;
      if (!fir_gen_plan(taps.data(), (int)taps.size(), s.R1, ph, &probe, &fr) || probe.pc > s.pct || probe.nb > s.nbt) { fits = false; }
    }
    if (!fits) { continue; }
    *R1_out = s.R1; *R2_out = R2; *wu_out = wu;
    return true;
  }
  return false;
}

// taps of stage 1: z^-(N-1) boxcar(R1)^N
void cic2_stage1_taps(int R1, int N, std::vector<int64_t> *h) {
  std::vector<int64_t> c(1, 1);
  for (int st = 0; st < N; st++) {
    std::vector<int64_t> nx(c.size() + R1 - 1, 0);
    for (size_t i = 0; i < c.size(); i++) { for (int j = 0; j < R1; j++) { nx[i + j] += c[i]; } }
    c.swap(nx);
  }
  h->assign((size_t)N - 1, 0);
  h->insert(h->end(), c.begin(), c.end());
}

// history samples a handle must keep in front of a call so that chunk 0's warm-up steps and first window are readable
int cic2_hist_len(int in_eb, int R1, int N, int wu) {
  const int ls = 8 / in_eb;
  return wu * 256 * R1 + (N * R1 + 15) + 16 * ls + 64;
}

static int cic2_batch(const Shape *sh) { return (sh && sh->m == 2) ? 4 : 2; }

// Steps per chunk, warm-up included.  A chunk pays `wu` steps of re-read and re-computed input and one pipeline start (fragments, halo,
// two load groups before the first product): 48 steps where a row holds at least two such chunks, 24 where it holds two of those, else 12
// (same-process sweep in profiles/r6_cic2_ablation.txt: 2.31 / 2.14 / 1.99 ms at 12 / 24 / 48 steps on 2^20-sample rows; 64 and 96 lose again
// to the uneven tail of rows that hold four or three chunks).
static int cic2_steps_per_chunk(const void *shape, int wu, int64_t steps_per_row) {
  const Shape *sh = (const Shape *)shape;
  const int g = cic2_batch(sh);
  ACDSP_TUNE_ENV(env, "ACDSP_CIC2_NST");   // tuning knob
  int nst = env && atoi(env) > 0 ? atoi(env) : (steps_per_row >= 2 * 47 ? 48 : (steps_per_row >= 2 * 23 ? 24 : 12));
  if (nst < wu + 1) { nst = wu + 1; }
  nst = (nst + g - 1) / g * g;
  if (nst > 96) { nst = 96; }
  return nst;
}

// Outputs [0, *covered) of the call are written; the caller runs the recurrence kernel on the rest (the ragged end of the call).
hipError_t launch_cic2(const CicParams &p, const FirGenPlan &pl, const uint32_t *d_frag, int R1, int R2, int wu, int64_t n_out,
                       hipStream_t s, int64_t *covered) {
  *covered = 0;
  const Shape *sh = find_shape(p.in_eb, R1);
  if (!sh || pl.pc > sh->pct || pl.nb > sh->nbt || pl.R != R1 || n_out <= 0) { return hipSuccess; }
  Cic2Args a;
  memset(&a, 0, sizeof a);
  a.pl = pl;
  a.n_ch = p.n_ch; a.N = p.N; a.me = p.me; a.R2 = R2; a.w_int = p.w_int;
  a.in_F = p.in.F; a.out = p.out; a.out_eb = p.out_eb; a.out_simple = p.out_simple;
  a.hl = p.hl;
  const int ls = 8 / p.in_eb;
  const int64_t w0slot = (p.first - pl.off) / 16;                    // exact: the plan aligns the window start to a slot
  a.ring_delta = (int32_t)(((w0slot % ls) + ls) % ls);
  a.wu = wu;
  a.rcp2 = (uint32_t)((0x100000000ull + R2 - 1) / R2);
  // pairwise recombination of the plane accumulators (fir_gen.hip: gen_fill_args)
  {
    const int px = p.in_eb;
    int64_t bw[16] = {0};
    for (int w = 0; w < px + pl.pc - 1; w++) {
      for (int q = 0; q < pl.pc; q++) { if (w - q >= 0 && w - q < px) { bw[w] += 128 * pl.dig_abs[q]; } }
    }
    bool ok = true;
    for (int w = 0; w + 1 < 16; w += 2) { ok = ok && (bw[w + 1] * 256 + bw[w] < (int64_t(1) << 31)); }
    static const bool no_pw = getenv("ACDSP_GEN_NO_PW") != nullptr;
    a.pw = (ok && !no_pw) ? 1 : 0;
    unsigned __int128 bias = 0;
    for (int q = 0; q < px - 1; q++) { bias += (unsigned __int128)1 << (8 * q); }
    // byte rows (px = 1) of an unsigned IN_TYPE: the kernel flips the sign bit of its only plane, x - 128, and reads a non-zero corr as the
    // order to do so (sum_h = R1^N > 0 and far below 2^57: 128 sum_h is never 0 mod 2^64)
    if (px == 1 && !p.in.S) { bias += 1; }
    a.corr = (int64_t)(unsigned long long)((unsigned __int128)128 * bias * (unsigned long long)pl.sum_h);
  }
  { ACDSP_TUNE_ENV(dbg_env, "ACDSP_CIC2_DBG"); a.dbg = dbg_env ? atoi(dbg_env) : 0; }
  a.first = p.first; a.n_out = n_out; a.n16 = (p.n_in + 15) / 16 * 16;
  a.in_stride = p.in_stride; a.out_stride = p.out_stride;
  a.x = p.x; a.y = p.y; a.hist = p.hist;
  // complete chunks only: every u of the chunk has its whole window inside the call's samples
  const int64_t u_valid = p.n_in > p.first ? (p.n_in - p.first + R1 - 1) / R1 : 0;     // u[m] needs x[first + m R1]
  a.nst = cic2_steps_per_chunk(sh, wu, u_valid / 256);
  const int nmain = a.nst - wu;
  const int64_t chunks = u_valid / (256 * (int64_t)nmain);
  // ... and one shorter chunk behind them for the end of the call (a whole number of load-group pairs)
  const int g = cic2_batch(sh);
  const int64_t rem_steps = u_valid / 256 - chunks * nmain;
  a.full_chunks = (int32_t)chunks;
  a.nst_last = (int32_t)((rem_steps + wu) / g * g);
  const int last_main = a.nst_last > wu ? a.nst_last - wu : 0;
  if (last_main == 0) { a.nst_last = 0; }
  if (chunks + (last_main > 0) < 1 || u_valid >= (int64_t(1) << 30) || chunks >= (int64_t(1) << 30)) { return hipSuccess; }
  // chunk 0 reads back to c0 = first - off - 16 delta - wu 256 R1
  if (-(p.first - pl.off - 16 * (int64_t)a.ring_delta - (int64_t)wu * 256 * R1) > p.hl) { return hipSuccess; }
  const int64_t fast_out = ((chunks * nmain + last_main) * 256 + R2 - 1) / R2;         // j R2 < u indices covered
  dim3 grid((unsigned)(chunks + (last_main > 0)), (unsigned)p.n_ch);
  // XCD-affine chunk order: -2 .. -4 % in the same-process sweeps (profiles/r6_cic2_ablation.txt); ACDSP_XCD_MAP=0 is the A/B knob
  a.xcd_map = (xcd_map_wanted(true) && ((int64_t)grid.x * grid.y) % 8 == 0) ? 1 : 0;
  const v4i *fr = (const v4i *)d_frag;
  hipError_t e = hipErrorInvalidValue;
  e = sh->launch(g, p.N, grid, s, a, fr);
  if (e != hipSuccess) { return e; }
  *covered = fast_out < n_out ? fast_out : n_out;
  return hipSuccess;
}
}  // namespace acdsp
