// wa_load_plan.h - how the model loader (wa_loader.cpp) cuts a tensor's bytes into the chunks that go through its staging buffers.
// Pure host arithmetic, no HIP include: tests/native/load_plan.cpp compiles it with g++ alone.
//
// A staging buffer holds `cap` bytes; `used` of them are taken by earlier tensors of the same fill.  A tensor of `nbytes` bytes in rows of
// `row_bytes` bytes is cut into chunks of WHOLE rows - a quantised block (22 .. 210 bytes) never straddles two chunks, and every unpack
// kernel sees a run of complete rows.  The first chunk takes the rows that still fit behind `used`; when not even one row fits there it is
// sized for an empty buffer instead, and so is every later chunk.  The caller starts a new buffer whenever a chunk does not fit behind what
// it has already placed (used + rows * row_bytes > cap), so the list says where to cut, and the caller's one rule says where to switch.
#pragma once
#include <cstddef>
#include <vector>

#define WA_LOAD_ALIGN 16        // a chunk starts at a multiple of this in its staging buffer (the conv kernel's 16-byte loads)

struct wa_load_chunk {
    size_t file_off;            // first byte of the chunk, counted from the tensor's first byte
    size_t row0;                // its first row
    size_t rows;                // its row count, at least 1
};

inline size_t wa_load_align(size_t bytes) { return (bytes + (WA_LOAD_ALIGN - 1)) & ~(size_t) (WA_LOAD_ALIGN - 1); }

// Empty when the arguments admit no plan: no bytes, rows that do not tile the tensor, a row larger than a whole buffer, used > cap.
inline std::vector<wa_load_chunk> wa_load_plan(size_t nbytes, size_t row_bytes, size_t cap, size_t used) {
    std::vector<wa_load_chunk> plan;
    if (nbytes == 0 || row_bytes == 0 || nbytes % row_bytes != 0 || row_bytes > cap || used > cap) return plan;
    const size_t n_rows = nbytes / row_bytes, per_buffer = cap / row_bytes;
    size_t fit = (cap - used) / row_bytes;
    if (fit == 0) fit = per_buffer;
    for (size_t row = 0; row < n_rows;) {
        const size_t rows = n_rows - row < fit ? n_rows - row : fit;
        plan.push_back({ row * row_bytes, row, rows });
        row += rows;
        fit = per_buffer;
    }
    return plan;
}
