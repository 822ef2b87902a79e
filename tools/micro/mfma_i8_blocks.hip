// Microtest: which lane feeds what, and which register holds what, in v_mfma_i32_16x16x4_4b_i8 (__builtin_amdgcn_mfma_i32_16x16x4i8) - four
// independent 16 x 16 products with K = 4 signed bytes in one instruction.  k_qgemm_mfma (whisper-rust_amd/csrc/wa_quant.hip) takes the block index
// for the lane-sum index of a quant block, so a swapped row, column or block there would be wrong numbers, not a fault: pin it here first.
//   hypothesis  A: lane L holds the four K-bytes of block L / 16, row L % 16
//               B: lane L holds the four K-bytes of block L / 16, column L % 16
//               D: register 4 blk + r of lane L is block blk, row 4 (L / 16) + r, column L % 16
// Pass 1, one-hot: A is all ones in ONE (block, row) and zero elsewhere, B all ones in ONE (block, column): the only non-zero output (= 4) names the
// (lane, register) of that (block, row, column) - and nothing may appear when the two blocks differ.  Every (block, row) x (block, column) pair.
// Pass 2, values: random signed bytes (-128 included), D against the host's four-term integer sums plus a C operand, every lane and register.
// Pass 3, K order: byte e of A meets byte e of B (one-hot bytes).
// Build: hipcc --offload-arch=gfx950 -O2 tools/micro/mfma_i8_blocks.hip -o mfma_i8_blocks    exit status 0 = the hypothesis holds
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
typedef int i32x16 __attribute__((ext_vector_type(16)));

// one wave; A, B: one int (four bytes) per lane; C, D: [lane][16]
__global__ void k_mfma_i8(const int * A, const int * B, const int * C, int * D) {
    const int l = threadIdx.x;
    i32x16 acc;
    for (int i = 0; i < 16; ++i) acc[i] = C[l * 16 + i];
    acc = __builtin_amdgcn_mfma_i32_16x16x4i8(A[l], B[l], acc, 0, 0, 0);
    for (int i = 0; i < 16; ++i) D[l * 16 + i] = acc[i];
}

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }
static int pack(const int8_t * b) { uint32_t v = 0; for (int e = 0; e < 4; ++e) v |= (uint32_t) (uint8_t) b[e] << (8 * e); return (int) v; }

int main() {
    int * dA, * dB, * dC, * dD;
    if (hipMalloc(&dA, 64 * 4) != hipSuccess || hipMalloc(&dB, 64 * 4) != hipSuccess || hipMalloc(&dC, 1024 * 4) != hipSuccess || hipMalloc(&dD, 1024 * 4) != hipSuccess) {
        fprintf(stderr, "no device memory\n"); return 2;
    }
    std::vector<int> A(64), B(64), Cc(1024), D(1024);
    auto run = [&]() {
        if (hipMemcpy(dA, A.data(), 256, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dB, B.data(), 256, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dC, Cc.data(), 4096, hipMemcpyHostToDevice) != hipSuccess) return false;
        hipLaunchKernelGGL(k_mfma_i8, dim3(1), dim3(64), 0, 0, dA, dB, dC, dD);
        return hipMemcpy(D.data(), dD, 4096, hipMemcpyDeviceToHost) == hipSuccess;
    };
    // the hypothesis: where (block, row, column) is found
    auto where = [](int blk, int row, int col, int & lane, int & reg) { lane = 16 * (row / 4) + col; reg = 4 * blk + (row % 4); };
    long bad = 0, n = 0;

    // pass 1: one-hot (block, row) x (block, column)
    int map_shown = 0;
    for (int ba = 0; ba < 4; ++ba) for (int row = 0; row < 16; ++row) for (int bb = 0; bb < 4; ++bb) for (int col = 0; col < 16; ++col) {
        std::fill(A.begin(), A.end(), 0); std::fill(B.begin(), B.end(), 0); std::fill(Cc.begin(), Cc.end(), 0);
        A[16 * ba + row] = 0x01010101; B[16 * bb + col] = 0x01010101;
        if (!run()) { fprintf(stderr, "HIP error\n"); return 2; }
        int lane, reg; where(ba, row, col, lane, reg);
        for (int i = 0; i < 1024; ++i) {
            const int want = (ba == bb && i == lane * 16 + reg) ? 4 : 0;
            ++n;
            if (D[i] != want) {
                if (bad < 10) printf("one-hot A(block %d, row %d) B(block %d, col %d): lane %d reg %d holds %d, hypothesis says %d\n", ba, row, bb, col, i / 16, i % 16, D[i], want);
                ++bad;
            }
        }
        if (ba == bb && col == 5 && (row == 0 || row == 6 || row == 15) && map_shown < 12) {
            for (int i = 0; i < 1024; ++i) if (D[i]) { printf("block %d row %2d col %2d -> lane %2d register %2d\n", ba, row, col, i / 16, i % 16); ++map_shown; }
        }
    }
    printf("one-hot pass: %ld outputs checked, %ld against the hypothesis\n", n, bad);

    // pass 2: random signed bytes and a C operand
    long bad2 = 0, n2 = 0;
    for (int t = 0; t < 64; ++t) {
        int8_t a[64][4], b[64][4];
        for (int l = 0; l < 64; ++l) for (int e = 0; e < 4; ++e) {
            a[l][e] = (int8_t) (t < 2 ? -128 : (int) (rnd() % 256) - 128);          // (-128) * (-128) * 4 = 65536: no saturation of a product or a sum
            b[l][e] = (int8_t) (t < 2 ? (t ? 127 : -128) : (int) (rnd() % 256) - 128);
        }
        for (int l = 0; l < 64; ++l) { A[l] = pack(a[l]); B[l] = pack(b[l]); }
        for (auto & v : Cc) v = (t & 1) ? (int) (rnd() % 2000001) - 1000000 : 0;
        if (!run()) { fprintf(stderr, "HIP error\n"); return 2; }
        for (int blk = 0; blk < 4; ++blk) for (int row = 0; row < 16; ++row) for (int col = 0; col < 16; ++col) {
            int lane, reg; where(blk, row, col, lane, reg);
            int want = Cc[lane * 16 + reg];
            for (int e = 0; e < 4; ++e) want += (int) a[16 * blk + row][e] * (int) b[16 * blk + col][e];
            ++n2;
            if (D[lane * 16 + reg] != want) { if (bad2 < 10) printf("values: block %d row %d col %d: got %d want %d\n", blk, row, col, D[lane * 16 + reg], want); ++bad2; }
        }
    }
    printf("value pass: %ld outputs checked, %ld wrong\n", n2, bad2);

    // pass 3: byte e of A meets byte e of B
    long bad3 = 0;
    for (int ea = 0; ea < 4; ++ea) for (int eb = 0; eb < 4; ++eb) {
        for (int l = 0; l < 64; ++l) { A[l] = 3 << (8 * ea); B[l] = 5 << (8 * eb); }
        std::fill(Cc.begin(), Cc.end(), 0);
        if (!run()) { fprintf(stderr, "HIP error\n"); return 2; }
        for (int i = 0; i < 1024; ++i) if (D[i] != (ea == eb ? 15 : 0)) ++bad3;
    }
    printf("K-byte pass: %ld wrong\n", bad3);
    printf((bad | bad2 | bad3) ? "HYPOTHESIS REFUTED\n" : "hypothesis confirmed: A lane L = (block L/16, row L%%16), B lane L = (block L/16, column L%%16), "
                                                          "D register 4 blk + r of lane L = (block blk, row 4 (L/16) + r, column L%%16)\n");
    return (bad | bad2 | bad3) ? 1 : 0;
}
