// tools/gen_select_walk.hip -- host-only walk of fir_gen_select (fir_gen.hip) over the plan grid: in_eb {1,2,4,8} x px 1..8 x pc 1..3 x nb 1..8 x
// oeb {2,4,8} x R 1..64 x lz {0,1} x conv_ok {0,1} x out_vec_ok {0,1} x ACDSP_GEN_RING {unset, "0", "2,2,1,0", "4,2,1,1", "1,1,1,0"}.
//   * every selected row's bounds must contain the plan (in_eb, px, pc <= pct, nb <= nbt, oeb, R, lz), byte rows (in_eb == 1) included;
//   * the selections of in_eb >= 2 are folded into one FNV-1a hash, printed with the case counts: the same program built against two
//     trees prints the same line when no unflagged selection differs (pass `words` to leave the in_eb == 1 half out on a tree without it).
// Build (host side under the sanitizers; no kernel is launched):
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -Xarch_host -fsanitize=address,undefined -Iac_dsp_amd/csrc tools/gen_select_walk.hip \
//         ac_dsp_amd/csrc/fir_gen.hip ac_dsp_amd/csrc/fir_gen_ring.hip ac_dsp_amd/csrc/fir_gen_ring_s8.hip -o tools/_bin/gen_select_walk
#include <cstdio>
#include <cstring>

#include "fir_gen_kernels.hpp"

using namespace acdsp;

int main(int argc, char **argv) {
  const bool words_only = argc > 1 && !strcmp(argv[1], "words");
  const char *envs[] = {nullptr, "0", "2,2,1,0", "4,2,1,1", "1,1,1,0"};
  const int ebs[] = {1, 2, 4, 8}, oebs[] = {2, 4, 8};
  unsigned long long hash = 1469598103934665603ull;
  auto fold = [&](long long v) { for (int i = 0; i < 8; i++) { hash = (hash ^ (unsigned long long)((v >> (8 * i)) & 0xff)) * 1099511628211ull; } };
  long long cases = 0, with_row = 0, byte_cases = 0, byte_with_row = 0, bad = 0;
  long long per_id[64] = {0};
  for (int eb : ebs) {
    if (eb == 1 && words_only) { continue; }
    for (int px = 1; px <= 8; px++) for (int pc = 1; pc <= 3; pc++) for (int nb = 1; nb <= 8; nb++) for (int oeb : oebs) for (int R = 1; R <= 64; R++)
    for (int lz = 0; lz < 2; lz++) for (int cv = 0; cv < 2; cv++) for (int ov = 0; ov < 2; ov++) for (const char *env : envs) {
      const GenSelect s = fir_gen_select(eb, px, pc, nb, oeb, R, lz != 0, cv != 0, ov != 0, env);
      if (s.row) {
        const RingRow &r = *s.row;
        if (r.in_eb != eb || r.px != s.px || pc > r.pct || nb > r.nbt || r.oeb != oeb || r.R != R || r.lz != lz || !cv || !ov) { bad++; }
      }
      if (eb == 1) {
        byte_cases++;
        if (s.row) { byte_with_row++; if (s.row->id >= 0 && s.row->id < 64) { per_id[s.row->id]++; } }
        if (s.nbt != 0 || (s.row && px != 1)) { bad++; }   // no window-per-step fast shape, and no row for more than one plane
      } else {
        cases++;
        if (s.row) { with_row++; }
        fold(s.row ? s.row->id : 0); fold(s.row ? s.row->nbt : 0); fold(s.row ? s.row->pct : 0); fold(s.nbt); fold(s.spw); fold(s.pf); fold(s.nt); fold(s.fb); fold(s.px);
      }
    }
  }
  printf("in_eb >= 2: %lld cases (%lld with a ring shape), selection hash %016llx\n", cases, with_row, hash);
  if (!words_only) {
    printf("in_eb == 1: %lld cases (%lld with a ring shape);", byte_cases, byte_with_row);
    for (int id = 0; id < 64; id++) { if (per_id[id]) { printf(" id %d: %lld", id, per_id[id]); } }
    printf("\n");
  }
  printf("rows whose bounds do not contain their plan: %lld\n", bad);
  return bad ? 1 : 0;
}
