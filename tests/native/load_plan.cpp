// load_plan.cpp - TEST INFRASTRUCTURE ONLY: the model loader's chunk planner (whisper-rust_amd/csrc/wa_load_plan.h, no HIP) behind a
// command line, for tests/test_load_plan_math.py.  g++ alone.
//   load_plan <cases.txt> : one case per line, "nbytes row_bytes cap used"; prints "plan <n>" and then n lines "file_off row0 rows" per case
#include "wa_load_plan.h"

#include <cstdio>

int main(int argc, char ** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    FILE * f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    unsigned long long nbytes, row_bytes, cap, used;
    while (fscanf(f, "%llu %llu %llu %llu", &nbytes, &row_bytes, &cap, &used) == 4) {
        const std::vector<wa_load_chunk> plan = wa_load_plan((size_t) nbytes, (size_t) row_bytes, (size_t) cap, (size_t) used);
        printf("plan %zu\n", plan.size());
        for (const wa_load_chunk & c : plan) printf("%zu %zu %zu\n", c.file_off, c.row0, c.rows);
    }
    fclose(f);
    return 0;
}
