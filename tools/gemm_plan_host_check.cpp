// Host check of the GEMM dispatch policy (csrc/gemm_plan.h), meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ifreepose_amd/csrc tools/gemm_plan_host_check.cpp -o gemm_plan_host_check
// Reads lines "M N K epi ldx ldw ln_part no_split ncu" on stdin and prints for each the text fp_op_gemm_plan writes for that launch
// under the product's options: "<label> row0=<r> ring=<a>,<b> grid=<a>,<b>".  On the way it holds every plan to what the launcher
// relies on: the parts tile the rows, a split falls on a tile boundary, rings and grids are inside the kernels' limits.
// tests/test_gemm_cases_cpu.py compares the output with the Python mirror of the dispatch (tests/_gemm_cases.py).
#include <stdio.h>

#include "gemm_plan.h"

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

int main() {
    using namespace fp_plan;
    static_assert(ring_max(64, 64, 1, false) == 8 && ring_max(64, 64, 2, true) == 8 && asm_big_lds(true) == LDS_BUDGET, "LDS geometry");
    static_assert(ncu_dispatch(256) == 256 && ncu_dispatch(304) == 304 && ncu_dispatch(20) == 16 && ncu_dispatch(0) == 256 && ncu_resident(20) == 20 &&
                      ncu_resident(8) == 256 && ncu_persistent(20) == 16, "CU count forms");
    Shape s{};
    int ln_part = 0, no_split = 0, n = 0;
    char text[160];
    while (scanf("%d %d %d %d %d %d %d %d %d", &s.M, &s.N, &s.K, &s.epi, &s.ldx, &s.ldw, &ln_part, &no_split, &n) == 9) {
        s.ln_part = ln_part != 0;
        s.no_split = no_split != 0;
        const Plan p = make_plan(s, n);
        CHECK(p.nparts == (p.split == SPLIT_NONE ? 1 : 2) && p.part[0].row0 == 0);
        int rows = 0;
        for (int i = 0; i < p.nparts; ++i) {
            const Part& q = p.part[i];
            CHECK(q.row0 == rows && q.rows > 0 && q.grid > 0);
            CHECK(q.tier == TINY64 ? (q.ring >= 2 && q.ring <= RING_CAP && q.ring <= (s.K / BK > 2 ? s.K / BK : 2)) : q.ring == 0);
            // a ring's whole grid is resident, and a persistent grid never exceeds the CUs
            if (q.ring > 2) CHECK((long)q.grid <= (long)ncu_resident(n) * (LDS_BUDGET / (fixed_bytes(tiny_waves(s.epi), epi_gelu(s.epi)) + q.ring * stage_bytes(64, 64))));
            if (q.tier >= BIG_HIP) CHECK(q.grid <= ncu_dispatch(n) && !(s.ln_part && !p.finalize_first));
            rows += q.rows;
        }
        CHECK(rows == s.M);
        if (p.split != SPLIT_NONE) CHECK(epi_row_major(s.epi) && !s.no_split && p.part[0].rows % (p.split == SPLIT_BIG ? 256 : 128) == 0);
        const int k = plan_text(p, text, sizeof text);
        CHECK(k > 0 && (size_t)k < sizeof text);
        puts(text);
    }
    if (fails) printf("%d checks FAILED\n", fails);
    return fails ? 1 : 0;
}
