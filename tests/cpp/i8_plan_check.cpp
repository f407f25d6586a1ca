// gemma_amd/csrc/i8_plan.h as a stand-alone host program (no HIP): it prints what the plan decides and judges nothing --
// tests/test_i8_plan_cpu.py holds the expected lines as literals and builds this plain and with -fsanitize=address,undefined.
//   i8_plan_check form [key=value ...]   one line: the form and the ordered launches of one product
//   i8_plan_check sweep                  that line for every combination of the switches and arguments, the inputs in front
//   i8_plan_check chunks [key=value ...] one line: i8_chunks for l
//   i8_plan_check pipe [key=value ...]   one line: i8_pipe_eligible for kind
// Keys: the members of I8Switches, and n, l, digits, have_map, allow_epi, allow_direct, kind.  What is not given is the default of
// I8Switches, n = 20000, l = 257, digits = 6, no indicator map, epilogue and direct form allowed, a PLINK block.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../gemma_amd/csrc/i8_plan.h"

using namespace gemma_hip;

struct Case {
  I8Switches k;
  size_t n = 20000, l = 257;
  int digits = 6, have_map = 0, allow_epi = 1, allow_direct = 1, kind = GEMMA_GENO_PLINK_2BIT;
};

static bool set_key(Case &c, const char *arg) {
  const char *eq = strchr(arg, '=');
  if (!eq) return false;
  const size_t len = (size_t)(eq - arg);
  const long v = atol(eq + 1);
  const struct { const char *name; int *at; } ints[] = {
      {"utx_i8", &c.k.utx_i8}, {"sparse", &c.k.sparse}, {"rows", &c.k.rows}, {"fuse", &c.k.fuse}, {"mdrop", &c.k.mdrop},
      {"complete", &c.k.complete}, {"epilogue", &c.k.epilogue}, {"epi_depth", &c.k.epi_depth}, {"direct", &c.k.direct},
      {"raster", &c.k.raster}, {"gm", &c.k.gm}, {"overlap", &c.k.overlap}, {"chunks", &c.k.chunks}, {"digits", &c.digits},
      {"have_map", &c.have_map}, {"allow_epi", &c.allow_epi}, {"allow_direct", &c.allow_direct}, {"kind", &c.kind}};
  for (const auto &e : ints)
    if (strlen(e.name) == len && strncmp(e.name, arg, len) == 0) return *e.at = (int)v, true;
  if (len == 1 && arg[0] == 'n') return c.n = (size_t)v, true;
  if (len == 1 && arg[0] == 'l') return c.l = (size_t)v, true;
  return false;
}

static void print_form(const Case &c) {
  static const char *const modes[] = {"dense", "bytes", "r32", "r16"};
  static const char *const kernels[I8K_COUNT] = {"packed<true>", "sparse", "sparse2", "r16", "r16_g", "r16_ep", "r16_ep_g"};
  const I8Form f = i8_form(c.k, c.n, c.l, c.digits, c.have_map != 0, c.allow_epi != 0, c.allow_direct != 0);
  I8Launch plan[4];
  const int launches = i8_launches(f, plan);
  printf("mode=%s fuse=%d digits=%d nplanes=%d c_planes=%d mdrop=%d complete=%d epi=%d direct=%d lpad=%zu mrows=%zu", modes[f.mode],
         f.fuse, f.digits, f.nplanes, f.c_planes, f.mdrop, f.complete, f.epi, f.direct, f.lpad, f.mrows);
  for (int i = 0; i < launches; ++i)
    printf(" | %s y%d p%d r%d%s", kernels[plan[i].kernel], plan[i].planes, plan[i].plane0, plan[i].run_if,
           plan[i].writes_utx ? " w" : "");
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  Case c;
  for (int i = 2; i < argc; ++i)
    if (!set_key(c, argv[i])) return fprintf(stderr, "bad argument %s\n", argv[i]), 2;
  if (strcmp(argv[1], "form") == 0) {
    print_form(c);
  } else if (strcmp(argv[1], "chunks") == 0) {
    printf("%d\n", i8_chunks(c.k, c.l));
  } else if (strcmp(argv[1], "pipe") == 0) {
    printf("%d\n", i8_pipe_eligible(c.k, c.kind) ? 1 : 0);
  } else if (strcmp(argv[1], "sweep") == 0) {
    const size_t ns[2] = {32640, 32641};
    for (int bits = 0; bits < 1 << 9; ++bits)
      for (int sparse = 0; sparse < 3; ++sparse)
        for (int rows = 16; rows <= 32; rows += 16)
          for (int digits = 6; digits <= 7; ++digits)
            for (size_t n : ns) {
              Case s;
              s.k.sparse = sparse; s.k.rows = rows; s.digits = digits; s.n = n;
              s.k.fuse = bits & 1; s.k.mdrop = bits >> 1 & 1; s.k.complete = bits >> 2 & 1; s.k.epilogue = bits >> 3 & 1;
              s.allow_epi = bits >> 4 & 1; s.have_map = bits >> 5 & 1; s.k.direct = bits >> 6 & 1; s.allow_direct = bits >> 7 & 1;
              s.l = (bits >> 8 & 1) ? 512 : 257;
              printf("sparse=%d rows=%d fuse=%d mdrop=%d complete=%d epilogue=%d digits=%d n=%zu allow_epi=%d have_map=%d direct=%d "
                     "allow_direct=%d l=%zu => ", sparse, rows, s.k.fuse, s.k.mdrop, s.k.complete, s.k.epilogue, digits, n, s.allow_epi,
                     s.have_map, s.k.direct, s.allow_direct, s.l);
              print_form(s);
            }
  } else {
    return 2;
  }
  return 0;
}
