// wlsqm_chunk.hpp — what the staged one-lane-per-case kernels share (fit_stage.hip, fit_stage_iter.hip, fit_accurate.hip): how the lanes
// of a wave divide a chunk of its 64 rows among themselves, and the LDS-DMA transfer of one load instruction's pieces.  Plain helpers: the
// register-staged fetches, the slot rings, the waits and the LDS images stay with the kernels that own them.
#pragma once
#include <hip/hip_runtime.h>

namespace wlsqm {

typedef double d2_ __attribute__((ext_vector_type(2)));               // one 16-byte piece

// A wave stages the rows of its 64 consecutive cases in chunks of CH neighbours: per case CH DIM coordinates and CH values, moved as
// 16-byte pieces.  One load instruction moves the chunks of XCPI (FCPI) WHOLE cases, XPC (FPC) consecutive lanes per case: lane l takes
// piece l % XPC of case l / XPC (+ i XCPI in instruction i), so a case's pieces are one contiguous run of a row and a lane's global
// offset is the same 32-bit register for every instruction and chunk.  2D at CH = 8: 8 cases x 8 instructions for the coordinates; 3D:
// 5 cases x 13 instructions, lanes 60..63 idle (and the last instruction carries 4 cases); the values: 16 cases x 4 instructions.
template <int DIM, int CH>
struct ChunkPieces {
    static constexpr int XPC = CH * DIM * 8 / 16, FPC = CH * 8 / 16;        // 16-byte pieces of one case's chunk: coordinates, values
    static constexpr int XCPI = 64 / XPC, XNI = (64 + XCPI - 1) / XCPI;     // whole cases per load instruction; instructions per chunk
    static constexpr int FCPI = 64 / FPC, FNI = 64 / FCPI;
    static_assert(64 % FCPI == 0, "value rows: whole instructions");
};

// One LDS-DMA transfer: lane l's 16 bytes at base + voffset go to LDS byte lds_addr + 16 l (lds_addr wave-uniform), no vector register
// in between.  M0 holds the LDS base of such a transfer; the compiler reserves the register and does not preserve it around a
// statement, so the statement that sets it saves and restores it, and the s_nop 0 is the wait state between a scalar write of M0 and
// the transfer that reads it.  The compiler does not count the transfer: the caller waits with its own s_waitcnt vmcnt.
__device__ __forceinline__ void lds_dma_b128(const unsigned voffset, const char* const base, const unsigned lds_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voffset), "s"(base), "s"(lds_addr) : "memory");
}

}  // namespace wlsqm
