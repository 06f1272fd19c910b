// te_buffer.h -- buffer addressing (buffer_load / buffer_store ... s[rsrc], s_off offen): a 128-bit descriptor built from
// wave-uniform values, a 32-bit per-lane byte offset and a scalar byte offset; accesses past `bytes` return 0 per dword / are
// dropped.  Plain accesses go through the builtins; the "hidden" ones are inline asm with hand-counted waits, and everything
// learnt about them on the hardware is written down HERE (users: te_attn_kb.hip, te_attn_rc.hip; the descriptor and the plain
// accesses also te_attn_fwd6.hip and te_attn_l6.h).  scripts/check_hidden_loads.py (tests/test_isa_hazards.py) checks the
// compiled ISA of every kernel that uses the hidden loads.
#pragma once

#include "te_common.h"

typedef __amdgpu_buffer_rsrc_t Rsrc;
__device__ __forceinline__ Rsrc make_rsrc(const float* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)bytes, 0x00020000);
}
// bytes of a strided [N, 64] view (row stride sn floats) from its first element
__device__ __forceinline__ unsigned view_bytes(int N, int64_t sn) { return ((unsigned)(N - 1) * (unsigned)sn + 64u) * 4u; }
__device__ __forceinline__ float ld32(Rsrc r, unsigned voff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, 0, 0));
}
__device__ __forceinline__ f32x4 ld128(Rsrc r, unsigned voff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0));
}
__device__ __forceinline__ void st32(float x, Rsrc r, unsigned voff) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, x), r, voff, 0, 0);
}

// Loads hipcc's s_waitcnt insertion does not see: across a loop back-edge it loses the age order of in-flight loads and waits
// vmcnt(0) at the first use of ANY of them -- a full drain of the prefetch pipeline once per tile.  A tile loop therefore issues
// all its global loads and stores as inline asm and waits with hand-counted s_waitcnt vmcnt(n), n = the number of YOUNGER LOADS
// in flight (stores are never counted: loads retire in order among themselves, and a store that retires late only makes the wait
// longer).  After the wait, TE_PIN makes the value's first use follow it in program order.  The destination is a reference: a
// register with such a load in flight must never be COPIED (hipcc does not know it is not yet valid), so the request names the
// register set the value will be consumed from.
__device__ __forceinline__ void ld128_hidden(f32x4& v, Rsrc r, unsigned voff) {
  asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=&v"(v) : "v"(voff), "s"(r));
}
__device__ __forceinline__ void ld32_hidden(float& v, Rsrc r, unsigned voff) {
  asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=&v"(v) : "v"(voff), "s"(r));
}
#define TE_VM_WAIT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
template <int N_>      // the same with a count that is a constant expression
__device__ __forceinline__ void vm_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory");
}
#define TE_PIN(v) asm volatile("" : "+v"(v))
// Stores the compiler's s_waitcnt insertion does not see.  With loads AND stores in flight hipcc assumes they may retire out of
// order and drains vmcnt to zero before every use of a loaded value; hidden, the loads alone are counted exactly.  Safe: vmcnt
// counts these stores too, so a wait hipcc computes for its loads can only wait longer than it thinks, never shorter (loads
// retire in order among themselves); the store data is read at issue (no expcnt for VMEM stores on gfx9+).
__device__ __forceinline__ void st128_hidden(f32x4 x, Rsrc r, unsigned voff) {
  // (s_nop: a store of more than 64 bits reads the upper half of its data one cycle late -- the VALU instruction that follows
  //  must not write those registers.  hipcc pads this hazard for its own stores, not for inline asm: without the wait state
  //  cam_q came back with the upper 8 bytes of some lanes' 16-byte pieces replaced by whatever was written next, sporadically)
  asm volatile("buffer_store_dwordx4 %0, %1, %2, 0 offen\n\ts_nop 1" : : "v"(x), "v"(voff), "s"(r));
}
__device__ __forceinline__ void st32_hidden(float x, Rsrc r, unsigned voff) {
  asm volatile("buffer_store_dword %0, %1, %2, 0 offen" : : "v"(x), "v"(voff), "s"(r));
}
