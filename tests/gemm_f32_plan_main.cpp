// The fp32 GEMM dispatch plan on the CPU (tests/test_gemm_f32_plan_cpu.py).  stdin, one call per line: M N K Kw epilogue a_vec w_vec c_al bias_al extra_al cfg tail s16;
// stdout, one line per call: the "+"-joined kernel names of its plan, M1 of a row split or of a mixed launch (else 0), row0:rows of each launch.
#include <stdio.h>
#include "gemm_f32_plan.h"

int main() {
    namespace P = gemm_f32_plan;
    P::Call c;
    int f[5];
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d", &c.M, &c.N, &c.K, &c.Kw, &c.epilogue, &f[0], &f[1], &f[2], &f[3], &f[4], &c.cfg, &c.tail, &c.s16) == 13) {
        c.a_vec = f[0]; c.w_vec = f[1]; c.c_al = f[2]; c.bias_al = f[3]; c.extra_al = f[4];
        const P::Plan p = P::plan(c);
        char name[64];
        for (int i = 0; i < p.n; ++i) {
            P::kernel_name(p.l[i], c.N, name, sizeof(name));
            printf("%s%s", i ? "+" : "", name);
        }
        printf(" %d", p.n == 2 ? p.l[0].rows : p.l[0].M1);
        for (int i = 0; i < p.n; ++i) printf(" %d:%d", p.l[i].row0, p.l[i].rows);
        printf("\n");
    }
    return 0;
}
