// pdp_wave.h - device primitives shared by the kernel families: range-checked buffer stores and loads of tiles, the uniform-row LDS gather,
// the release signal between the two waves of a pair, and the compiler barriers.  What more than one family uses lives here, once; what one
// kernel alone needs stays in that kernel's header.
#pragma once
#include "pdp_tile.h"

namespace pdp {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---- range-checked buffer stores and loads
// Branch-free stores of tiles into exact-size arrays through BUFFER instructions: every lane keeps, per tile register, the byte offset of its element
// inside one time step's block - or BUF_OOB if the array has no such element, which the buffer's range check drops in hardware (and returns 0 for in a
// load; num_records = the trajectory's bytes of that array, far below 2 GB; 0 for an absent array, an output that was not asked for: everything dropped);
// the time step is the instruction's scalar offset.  store_map's predicated stores (pdp_tile.h) cost a basic block each (mask reload, branch, 64-bit
// address arithmetic) - ~20 per backward step of the lqrSolver kernel.
constexpr unsigned BUF_OOB = 0x80000000u;
// the resource of `bytes` bytes at `ptr`; a macro, because the same call inside an inline function changed the instruction schedule of the lqrSolver kernels
#define PDP_BUF_RSRC(ptr, bytes) __builtin_amdgcn_make_buffer_rsrc((void*)(ptr), 0, (int)(bytes), 0x00020000)
// byte offsets of a tile's elements; the builders encode each kernel's layout and stay with their kernels
struct BufMap { unsigned voff[4]; };
template <class RS>
PDP_DEV void buf_store_f64(RS rs, unsigned soff, unsigned voff, double x) {
    u32x2 w;
    w.x = (unsigned)__double2loint(x); w.y = (unsigned)__double2hiint(x);
    __builtin_amdgcn_raw_buffer_store_b64(w, rs, voff, soff, 0);
}
template <class RS>
PDP_DEV void buf_store_f64x2(RS rs, unsigned soff, unsigned voff, double x0, double x1) {
    u32x4 w;
    w.x = (unsigned)__double2loint(x0); w.y = (unsigned)__double2hiint(x0);
    w.z = (unsigned)__double2loint(x1); w.w = (unsigned)__double2hiint(x1);
    __builtin_amdgcn_raw_buffer_store_b128(w, rs, voff, soff, 0);
}
// (the store is spelled out here: a call of buf_store_f64 changed the instruction schedule of the lqrSolver kernels as well)
template <int NR = 4, class RS>
PDP_DEV void buf_store(RS rs, unsigned soff, const BufMap& m, const d4 v) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const double x = v[r];          // (through a scalar copy: bit-casting the vector element directly made every store write register 0's value; DESIGN.md section 8, finding 5)
        u32x2 w;
        w.x = (unsigned)__double2loint(x); w.y = (unsigned)__double2hiint(x);
        __builtin_amdgcn_raw_buffer_store_b64(w, rs, m.voff[r], soff, 0);
    }
}
template <int NR = 4, class RS>
PDP_DEV d4 buf_load(RS rs, unsigned soff, const BufMap& m) {
    d4 v = zero4();
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(rs, m.voff[r], soff, 0);
        v[r] = __hiloint2double((int)w.y, (int)w.x);
    }
    return v;
}

// ---- uniform-row LDS gather
// LDS addresses are kept ABSOLUTE (the base of the dynamic LDS block is a link-time constant the compiler cannot fold: added once, not as a VALU add in
// front of every ds_read); the ds_read / ds_write address is the register itself
#define PDP_LDS __attribute__((address_space(3)))
PDP_DEV unsigned lds_addr(const double* p) { return (unsigned)(uintptr_t)(PDP_LDS const double*)p; }
// Gathers over uniform rows: off[r] = slot (in doubles, inside a row) of tile element (lane, r); absent elements read the row's 0.0
struct RowGather { int off[4]; };
template <class CodeFn>
PDP_DEV void make_row_gather(RowGather& g, int lane, int c0, CodeFn code_of /* (row, col) -> code >= 0, -1 (zero) or <= -2 (constant) */) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int code = code_of(tile_row(lane, r), tile_col(lane));
        g.off[r] = code >= 0 ? code : (code == -1 ? c0 : c0 + 1 + (-2 - code));
    }
}
struct RowRun { unsigned cur[4]; };     // absolute LDS byte addresses of the four elements in the row the run is positioned at
PDP_DEV RowRun row_run_at(const RowGather& g, const double* row) {
    RowRun r;
    const unsigned base = lds_addr(row);
#pragma unroll
    for (int k = 0; k < 4; ++k) r.cur[k] = base + 8u * (unsigned)g.off[k];
    return r;
}
template <int NR = 4>
PDP_DEV d4 row_read(const RowRun& r, unsigned imm) {      // imm: byte distance of the wanted row from the run's row - a literal after unrolling
    d4 v = zero4();
#pragma unroll
    for (int k = 0; k < NR; ++k) v[k] = *(PDP_LDS const double*)(uintptr_t)(r.cur[k] + imm);
    return v;
}
template <int NR = 4>
PDP_DEV void row_move(RowRun& r, int bytes) {
#pragma unroll
    for (int k = 0; k < NR; ++k) r.cur[k] += (unsigned)bytes;
}

// ---- hand-over counters in LDS between the two waves of a pair
// release / acquire at workgroup scope (LDS and - for data a wave leaves in global memory - the CU's L1)
PDP_DEV void wg_signal(int* f, int v) { __hip_atomic_store(f, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
PDP_DEV void wg_wait_ge(int* f, int v) {
    while (__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < v) __builtin_amdgcn_s_sleep(2);
}

// ---- compiler barriers
// Mailbox values come out of LDS in vector registers although every lane reads the same word: said explicitly (v_readfirstlane), or every pointer and
// branch derived from them would be treated as divergent - 64-bit per-lane addresses for each of the OC solver's trial pass's ~100 loads, masked branches
// in its runner's control flow
PDP_DEV int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
PDP_DEV double uni(double v) { return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v))); }
// A value the optimiser cannot see through: per-lane maps derived from opaque(lane) INSIDE a sweep are recomputed at every sweep (a few hundred cycles against
// the sweep's 50 - 100 k) instead of being hoisted out of the iteration loop, where the maps of BOTH sweeps stayed live across each other and pushed the
// four-trajectories-per-workgroup instantiation (256 registers per wave) into scratch memory (round 3: 21 spilled VGPRs)
PDP_DEV int opaque(int v) { asm volatile("" : "+v"(v)); return v; }
// the same for values that live in SCALAR registers (launch constants: T, the workspace pointers).  Row offsets and row pointers derived from the plain T + 1 or from `stp`
// are invariants of the whole launch: the compiler forms all of them at kernel entry - two scalar registers per row pointer, 2 NX + NU rows per array - and keeps them, i.e.
// parks them in lanes of vector registers (round 6: FOUR vector registers of the four-trajectory instantiation held ~200 such words, read back ~1000 times).  Derived from an
// opaque copy inside a pass they are formed there (a few scalar instructions beside thousands of vector ones) and die with it.
PDP_DEV int sopaque(int v) { asm volatile("" : "+s"(v)); return v; }
template <class P> PDP_DEV P* sopaque(P* p) { asm volatile("" : "+s"(p)); return p; }

}  // namespace pdp
