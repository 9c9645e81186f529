// hopo_device.hip -- HIP/CDNA4 (gfx950) kernels and the thin C-ABI layer (tjamd_*) of the homopolymer-tract engine.
//
// Replaces, on the device, tatajuba's per-read scan (reference: src/hopo_counter.c:219-258,285-307) and the per-sample
// sort / dedupe / filter / index / coverage (reference: src/hopo_counter.c:339-438).  Integer and byte work only:
// HBM-bound, no MFMA.  See DESIGN.md for the data layout and the roofline of each kernel.
//
// Scan kernel in one paragraph: a workgroup (512 threads = 8 wavefronts, three resident per CU) takes tiles of 8 KiB of
// the '\n'-delimited read stream from a work counter.  The next tile's bytes go from HBM straight into LDS
// (global_load_lds, 1 KiB per wave instruction) while the current one is worked on.  Every lane classifies its 16 bytes
// with SWAR bit logic into 2-bit base codes plus three bit-planes (run start, read delimiter, non-ACGTU) kept in LDS.
// Run starts that begin a tract of >= m bases are found with shifted ANDs of the run-start plane, compacted into a
// workgroup-wide candidate list, and then one lane per candidate finds the run end (count-trailing-zeros on the plane),
// checks both flanks against the delimiter plane, pulls the two k-mers out of the packed codes with funnel shifts,
// canonicalises (reverse complement = bit reverse + pair swap of the complemented word) and appends a packed 8/16/32
// byte record to an LDS staging buffer, which the workgroup partitions into 256 hash buckets in HBM with one counting
// sort per few thousand records.  The finalise step aggregates every bucket in an LDS hash table (one workgroup per
// bucket), orders the survivors with a bin partition + per-wavefront rank sort, and derives the index and the coverage
// in the same pass.  File map: helpers and tile scan (scan_tiles) -> sinks (located list, bucket staging) -> bucket
// storage -> aggregation kernels -> radix sort / scans (fallback paths, merge) -> bin kernels -> host layer (tjamd_*).
// One program: the file has no preprocessor conditionals.  Tile sizes and occupancies are plain #defines, and the
// Makefile makes a -D that redefines one an error (-Werror=macro-redefined) instead of another library.

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>                  // types only: the library is looked up at run time (rccl_api)
#include <dlfcn.h>
#include <mutex>
#include <string>
#include <new>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdarg.h>
#include <limits.h>
#include <float.h>
#include <algorithm>
#include <vector>
#include <memory>

#include "../../include/tatajuba_amd.h"
#include "../../include/tatajuba_variants.h"
#include "../../include/tatajuba_features.h"
#include "../../include/tatajuba_effects.h"
#include "../../include/tatajuba_sites.h"
#include "../../include/tatajuba_depths.h"
#include "../../include/tatajuba_distances.h"
#include "../../include/tatajuba_linkage.h"
#include "../../include/tatajuba_agglomerate.h"
#include "../../include/tatajuba_groups.h"
#include "../../include/tatajuba_clades.h"
#include "../../include/tatajuba_bootstrap.h"
#include "../../include/tatajuba_replicate_trees.h"
#include "../../include/tatajuba_consensus.h"
#include "../../include/tatajuba_locate.h"

typedef unsigned long long u64;
typedef unsigned int u32;

// ---------------------------------------------------------------------------------------------------------------
// error plumbing

static thread_local char g_err[512] = "";

static int set_err (int code, const char *fmt, ...)
{
  va_list ap;
  va_start (ap, fmt);
  vsnprintf (g_err, sizeof (g_err), fmt, ap);
  va_end (ap);
  return code;
}

#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
  return set_err (TJAMD_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString (e_), __FILE__, __LINE__); } while (0)
#define HIPCHK_NULL(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
  set_err (TJAMD_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString (e_), __FILE__, __LINE__); return NULL; } } while (0)

extern "C" const char *tjamd_last_error (void) { return g_err; }
// (for the C half of the library, hopo_host.c; not exported)
extern "C" void tj_set_last_error (const char *msg) { (void) set_err (TJAMD_ERR_ARG, "%s", msg ? msg : "error"); }

extern "C" int tjamd_device_count (void)
{
  int n = 0;
  if (hipGetDeviceCount (&n) != hipSuccess) return 0;
  return n;
}

// ---------------------------------------------------------------------------------------------------------------
// geometry of the scan tile

#define TJ_HL      64                   // left halo  (>= max k + 1, multiple of 32)
#define TJ_HR      192                  // right halo (tracts whose end + k stays inside are handled from LDS)

template <int BLOCK, int TILE, int CANDDIV = 2>
struct TileLds
{
  static constexpr int WIN = TJ_HL + TILE + TJ_HR;       // bytes of stream seen by one tile
  static constexpr int NCHUNK = WIN / 16;                // 16-byte chunks
  static constexpr int MASKW = WIN / 32 + 4;             // words per bit-plane (+ zeroed pad for 3-word funnel reads)
  static constexpr int CODEW = WIN / 16 + 4;             // words of 2-bit codes (+ pad)
  static constexpr int MAXCAND = TILE / CANDDIV;         // tracts have >= 2 bases: one candidate per 2 bytes at most
                                                         // (CANDDIV 1: the located kernel's all-monomers mode)
  static constexpr int NLOAD = (NCHUNK + BLOCK - 1) / BLOCK;
  static constexpr int NRAW = NCHUNK + NLOAD * (BLOCK / 64);   // landing zone: the chunks + per wave and load, the chunk in front of its first one
  u32 code[CODEW];
  u32 start[MASKW];
  u32 sent[MASKW];
  u32 inval[MASKW];
  unsigned short cand[MAXCAND];
  u32 ncand;
  u32 grp[2];                                            // first tile of the current / next group of this workgroup
  u32 odd[2];                                            // per tile parity: some byte of the tile is neither ACGT nor '\n'
};

struct DevCounters
{
  u64 n_rec;        // records appended to the located list
  u64 n_fix_unused;
  u64 n_undefined;  // qualifying non-ACGTU runs without an earlier tract in the read (reference: uninitialised memory)
  u64 n_null;       // padding records written into the buckets (reserved slots that stayed empty)
  u32 overflow;     // output list / a bucket too small
  u32 fix_overflow; // fix list too small
  u32 pad[2];
  // per-launch counters, double-buffered: launch i works on lc[i & 1] and zeroes lc[(i + 1) & 1] for the next launch
  // (no memset between launches)
  // work = tile counter of the main scan kernel of the launch; n_slow = tiles the fast kernel handed to the generic one
  // (stream edges, bytes outside ACGT\n, too many candidates); work_slow = the generic kernel's counter over that list
  struct { u64 n_fix; u32 work, n_slow, work_slow, ticket, pad[2]; } lc[2];   // (ticket: workgroups of the generic kernel that are through, see scan_bins_kernel)
};

#define TJ_TILE_GROUP 16

struct FixEntry { long long pos; long long len; };

// counts of the finalise step (device block read back by the host)
struct FinCounts { u32 n_seg, n_kept, n_ctx, n_idx; int coverage; u32 overflow, sort_fallback, pad; };
// The sizes the ordering kernels work with, derived on the device from the number of kept records so that the host does
// not have to fetch that number between the aggregation and them (plan_tail; ok = 0: nothing to do, or more records
// than the buffers were sized for -- every kernel then returns at once and the host takes the exact path).
struct FinPlan { long n1; long t; int nbits, nbins, log2t, ok; u32 kept_overflow, cov_direct; long n1_exact; u32 ovf_exact, pad2; };   // (n1_exact, ovf_exact: read at the kernel boundary after the aggregation, see clear_buckets_kernel)


// ---------------------------------------------------------------------------------------------------------------
// device helpers

__device__ __forceinline__ u32 zero_bytes (u32 t)
{ // 0x80 in every byte of t that is zero, exact (no borrow between bytes)
  return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
}

__device__ __forceinline__ u32 gather_bit7 (u32 z)
{ // bit 7 of byte j -> bit j
  return ((z >> 7) | (z >> 14) | (z >> 21) | (z >> 28)) & 0xFu;
}

// Four stream bytes (x, byte 0 = lowest address) -> 8 bits of 2-bit codes, and 4-bit planes.
// Codes follow the reference's table (src/hopo_counter.c:205-216): A/a 0, C/c 1, G/g 2, T/t/U/u 3; every other byte is
// "other" and packs as 0 (reference :304-305 masks the table value 4 with 3).
__device__ __forceinline__ void classify_word (u32 x, u32 prev_byte, u32 &code8, u32 &start4, u32 &sent4, u32 &inval4)
{
  u32 a1 = x >> 1, a2 = x >> 2, a3 = x >> 3, a4 = x >> 4, a6 = x >> 6, a7 = x >> 7;
  // ACGTU in either case, as a boolean function of the byte's bits evaluated at bit 0 of every byte:
  // 0x41/43/47 (low nibble 1,3,7 with bit4 = 0) or 0x54/55 (low nibble 4,5 with bit4 = 1), bit5 free, bit6 = 1, bit7 = 0
  u32 v = ~a7 & a6 & ~a3 & ((~a4 & x & ~(a2 & ~a1)) | (a4 & a2 & ~a1));
  v &= 0x01010101u;
  u32 c = (a1 ^ a2) & (v * 3u);                       // ((b>>1)^(b>>2))&3 is the code of a valid byte
  code8 = (c | (c >> 6) | (c >> 12) | (c >> 18)) & 0xFFu;
  u32 iv = v ^ 0x01010101u;
  inval4 = (iv | (iv >> 7) | (iv >> 14) | (iv >> 21)) & 0xFu;
  sent4 = gather_bit7 (zero_bytes (x ^ 0x0A0A0A0Au));
  start4 = gather_bit7 (zero_bytes (x ^ ((x << 8) | prev_byte))) ^ 0xFu;   // run start: byte differs from its predecessor
}

// Fast path of classify_word for the bytes that make up almost all of a read stream: upper-case A C G T and the read
// delimiter.  Same code / start / delimiter planes (the code of a delimiter byte is never used); `bad` comes back non-zero if some byte is anything else (then the
// caller redoes the chunk with classify_word, which also produces the non-ACGTU plane).
// `hi` selects the weights 16..128 and the results are added to the incoming start4 / sent4: two words give one byte of
// each plane through the dot product's accumulator, without a merge instruction.
__device__ __forceinline__ void classify_word_fast (u32 x, u32 prev_word, bool hi, u32 &code8, u32 &start4, u32 &sent4, u32 &bad)
{
  const u32 wts = hi ? 0x80402010u : 0x08040201u;
  // 2-bit codes, packed with one dot product (byte j * 4^j)
  const u32 c = ((x >> 1) ^ (x >> 2)) & 0x03030303u;
  code8 = __builtin_amdgcn_udot4 (c, 0x40100401u, 0u, false);
  // delimiter: the only byte of the fast path without bit 6
  const u32 s = ~(x >> 6) & 0x01010101u;                 // (shift first: the and-not is then one instruction)
  sent4 = __builtin_amdgcn_udot4 (s, wts, sent4, false);
  // validation: every byte must be the letter its code stands for, or '\n' where bit 6 is clear -- one 8-entry byte
  // table look-up (v_perm_b32): entries 0..3 = 'A','C','G','T' by code, entries 4..7 = '\n'
  bad = x ^ __builtin_amdgcn_perm (0x0A0A0A0Au, 0x54474341u, c | (s << 2));
  // run start: byte differs from its predecessor
  const u32 d = x ^ __builtin_amdgcn_alignbit (x, prev_word, 24);
  // (the flag stays in bit 7 of its byte: the sum comes out 128 times too large and the caller's merge shift absorbs it)
  const u32 nz = (((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u;
  start4 = __builtin_amdgcn_udot4 (nz, wts, start4, false);
}

// inclusive prefix sum over the 64 lanes of a wavefront with DPP adds (row shifts inside 16-lane rows, then the two
// row broadcasts): 6 VALU instructions instead of 6 ds_bpermute round trips
__device__ __forceinline__ u32 wave_inclusive_scan (u32 x)
{
  x += (u32) __builtin_amdgcn_update_dpp (0, (int) x, 0x111, 0xF, 0xF, true);   // row_shr:1
  x += (u32) __builtin_amdgcn_update_dpp (0, (int) x, 0x112, 0xF, 0xF, true);   // row_shr:2
  x += (u32) __builtin_amdgcn_update_dpp (0, (int) x, 0x114, 0xF, 0xF, true);   // row_shr:4
  x += (u32) __builtin_amdgcn_update_dpp (0, (int) x, 0x118, 0xF, 0xF, true);   // row_shr:8
  x += (u32) __builtin_amdgcn_update_dpp (0, (int) x, 0x142, 0xA, 0xF, true);   // row_bcast:15 -> rows 1 and 3
  x += (u32) __builtin_amdgcn_update_dpp (0, (int) x, 0x143, 0xC, 0xF, true);   // row_bcast:31 -> rows 2 and 3
  return x;
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the wave's outstanding global stores and
// atomics (vmcnt(0), microseconds each under load); inside the scan nothing written to HBM is read back in the same
// launch, so the bucket writes and the cursor atomics are left in flight across barriers.
__device__ __forceinline__ void lds_barrier ()
{
  asm volatile ("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

typedef __attribute__((address_space(1))) const void *gptr_t;
typedef __attribute__((address_space(3))) void *lptr_t;
// LDS atomic add of a wave-uniform value by the wave's first lane alone, result left in flight: *raw_out (lane 0) holds
// the old value once lgkmcnt has drained (lds_collect).  Hand-written because the compiler's version of "one lane adds
// for the wave" costs a dozen scalar instructions, which on this chip are no cheaper than vector ones.
__device__ __forceinline__ void lds_add_issue (u32 lds_addr, u32 value_uniform, u32 &raw_out)
{
  u64 saved; u32 tmp;
  asm volatile ("s_mov_b64 %0, exec\n\ts_mov_b64 exec, 1\n\tv_mov_b32 %1, %4\n\tds_add_rtn_u32 %2, %3, %1\n\ts_mov_b64 exec, %0"
                : "=&s"(saved), "=&v"(tmp), "=&v"(raw_out) : "v"(lds_addr), "s"(value_uniform) : "memory");
}
__device__ __forceinline__ u32 lds_collect (u32 raw)
{
  asm volatile ("s_waitcnt lgkmcnt(0)" : "+v"(raw) :: "memory");
  return (u32) __builtin_amdgcn_readfirstlane ((int) raw);
}

// 64 bits of a little-endian bit array starting at bit position `bitpos` (array padded by >= 2 words)
__device__ __forceinline__ u64 bits64 (const u32 *a, int bitpos)
{
  int w = bitpos >> 5, sh = bitpos & 31;
  u32 x0 = a[w], x1 = a[w + 1], x2 = a[w + 2];
  u32 lo = __funnelshift_r (x0, x1, sh);
  u32 hi = __funnelshift_r (x1, x2, sh);
  return ((u64) hi << 32) | lo;
}

// 32 bits of a bit array starting at bit position `bitpos` (array padded by >= 1 word)
__device__ __forceinline__ u32 bits32 (const u32 *a, int bitpos)
{
  const int w = bitpos >> 5;
  return __builtin_amdgcn_alignbit (a[w + 1], a[w], (u32) bitpos & 31u);
}

// reverse complement of a k-mer of at most 16 bases held in 32 bits
__device__ __forceinline__ u32 revcomp_k32 (u32 x, int k)
{
  const u32 y = __brev (~x);
  u32 z;                                                // pair swap = bit-field insert of y >> 1 (even bits) into y << 1; the
  asm ("v_bfi_b32 %0, %1, %2, %3" : "=v"(z) : "s"(0x55555555u), "v"(y >> 1), "v"(y << 1));   // compiler spends 5 instructions on it
  return z >> (32 - 2 * k);
}

__device__ __forceinline__ u64 kmask (int k) { return (k >= 32) ? ~0ull : ((1ull << (2 * k)) - 1ull); }

// reverse complement of a k-mer packed first-base-lowest (reference: src/hopo_counter.c:241-242 builds it base by base)
__device__ __forceinline__ u64 revcomp_k (u64 x, int k)
{
  const u64 y = __brevll (~x);
  const u32 lo = (u32) y, hi = (u32) (y >> 32);
  u32 zl, zh;                                           // the pair swap never crosses the 32-bit halves: one v_bfi_b32 each
  asm ("v_bfi_b32 %0, %1, %2, %3" : "=v"(zl) : "s"(0x55555555u), "v"(lo >> 1), "v"(lo << 1));
  asm ("v_bfi_b32 %0, %1, %2, %3" : "=v"(zh) : "s"(0x55555555u), "v"(hi >> 1), "v"(hi << 1));
  return (((u64) zh << 32) | zl) >> (64 - 2 * k);
}

__device__ __forceinline__ u32 stream_byte (const uint8_t *seq, long n, long p)
{ // outside the stream everything is a read delimiter
  return (p >= 0 && p < n) ? (u32) seq[p] : (u32) '\n';
}

__device__ __forceinline__ bool byte_is_acgtu (u32 b)
{
  u32 l = b | 0x20u;
  return l == 'a' || l == 'c' || l == 'g' || l == 't' || l == 'u';
}

__device__ __forceinline__ u32 byte_code (u32 b) { return byte_is_acgtu (b) ? (((b >> 1) ^ (b >> 2)) & 3u) : 0u; }

// bit i of x -> bits 2i and 2i+1 (both set)
__device__ __forceinline__ u64 spread_pairs (u32 x)
{
  u64 v = x;
  v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
  v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
  v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
  v = (v | (v << 2)) & 0x3333333333333333ull;
  v = (v | (v << 1)) & 0x5555555555555555ull;
  return v | (v << 1);
}

// canonical record fields from the two flanks as read (reference: src/hopo_counter.c:233-246).  linv / rinv mark the
// non-ACGTU flank positions (k-bit masks): the reference's table gives them 4 in BOTH columns, so they pack as 0 in the
// reverse-complemented orientation too -- force their forward code to 3 before complementing.
__device__ __forceinline__ void canonicalise (u64 left, u64 right, u32 linv, u32 rinv, u32 cb, int k,
                                              u64 &c0, u64 &c1, u32 &base, u32 &flag)
{
  if (cb < 2u) { c0 = left; c1 = right; base = cb; flag = 1u; }
  else {
    if (linv | rinv) { left |= spread_pairs (linv); right |= spread_pairs (rinv); }
    c0 = revcomp_k (right, k); c1 = revcomp_k (left, k); base = 3u - cb; flag = 2u;
  }
}

__device__ __forceinline__ u64 make_meta (u32 base, long len, u32 flag)
{ // reference: src/hopo_counter.c:293-302 (count 1, mismatches 0xffe, multi 0, neg_strand 0), 10-bit length store
  return (u64) base | (((u64) len & 0x3FFull) << TJ_META_LEN_SHIFT) | TJ_META_RAW_CONST | ((u64) flag << TJ_META_FLAG_SHIFT);
}

// Slow path from global memory for a run [gs, ge] of a valid base: both flanks present?  then build the flanks.
__device__ bool flanks_from_stream (const uint8_t *seq, long n, long gs, long ge, int k, u64 &left, u64 &right, u32 &linv, u32 &rinv)
{
  left = right = 0; linv = rinv = 0;
  for (int i = 0; i < k; i++) {
    u32 bl = stream_byte (seq, n, gs - k + i), br = stream_byte (seq, n, ge + 1 + i);
    if (bl == '\n' || br == '\n') return false;
    left |= (u64) byte_code (bl) << (2 * i);
    right |= (u64) byte_code (br) << (2 * i);
    linv |= (byte_is_acgtu (bl) ? 0u : 1u) << i;
    rinv |= (byte_is_acgtu (br) ? 0u : 1u) << i;
  }
  return true;
}

template <int W>
__device__ __forceinline__ void store_record (u64 *out, u64 idx, u64 c0, u64 c1, u64 meta, u64 pos)
{
  u64 *p = out + idx * W;
  p[0] = c0; p[1] = c1; p[2] = meta;
  if (W == 4) p[3] = pos;
}

// wave-aggregated append: one atomic per wavefront, lanes ranked by ballot prefix (must be called wave-uniformly)
template <int W>
__device__ __forceinline__ void emit_record (bool have, u64 c0, u64 c1, u64 meta, u64 pos, u64 *out, u64 cap, DevCounters *ctr)
{
  u64 mask = __ballot (have);
  if (!mask) return;
  int lane = threadIdx.x & 63;
  int leader = __ffsll ((long long) mask) - 1;
  u64 base = 0;
  if (lane == leader) base = atomicAdd (&ctr->n_rec, (u64) __popcll (mask));
  base = __shfl (base, leader);
  if (have) {
    u64 idx = base + (u64) __popcll (mask & ((1ull << lane) - 1ull));
    if (idx < cap) store_record<W> (out, idx, c0, c1, meta, pos);
    else ctr->overflow = 1u;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// tile scan, shared by both kernels.  The sink receives, once per round and from every thread of the workgroup
// (wave- and block-uniform call), at most one tract: (have, ctx0, ctx1, base, 10-bit length, strand flag, position).

// Prefetch of one 16-byte chunk per lane straight into LDS (global_load_lds_dwordx4: no VGPR destination, so nothing
// the register allocator can turn into a copy that waits for the data).  lds_wave_base is the slot of the wave's first
// lane; lane l's 16 bytes land at lds_wave_base + l.  A chunk that sticks out of the stream reads the stream's first
// bytes instead and is rebuilt bytewise when it is consumed.  Requires >= 16 readable bytes at seq (the host pads tiny
// streams).

// The LDS-DMA instruction itself, from inline assembly.  Through the builtin the compiler knows that a VMEM operation
// writes LDS and, unable to tell where, waits for it (s_waitcnt vmcnt(0): the prefetch AND every bucket store in
// flight) in front of LDS accesses all over phases 2 and 3 -- the prefetch was complete a few hundred cycles after its
// issue instead of a tile later.  Unknown to the compiler, it is waited for exactly once, by the explicit s_waitcnt in
// front of phase 1's reads of the landing zone.  (Hidden VMEM operations can only make the compiler's own vmcnt waits
// longer, never shorter: the counter returns in issue order.)  lds_wave_base must be wave-uniform.
__device__ __forceinline__ void lds_dma16 (const void *gptr, void *lds_wave_base)
{
  const u32 m0v = (u32) __builtin_amdgcn_readfirstlane ((int) (u32) (size_t) (lptr_t) lds_wave_base);
  u32 saved;                                            // (M0 is the compiler's: put it back)
  asm volatile ("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                : "=&s"(saved) : "v"(gptr), "s"(m0v) : "memory");
}
__device__ __forceinline__ void issue_chunk (const uint8_t *__restrict__ seq, long n_bytes, long g, uint4 *lds_wave_base)
{
  const bool inside = (g >= 0) && (g + 16 <= n_bytes);
  lds_dma16 (inside ? seq + g : seq, lds_wave_base);
}

// the same chunk, byte by byte, for chunks that are not entirely inside the stream (first and last tile only)
struct EdgeChunk { u32 x, y, z, w; };
__device__ __noinline__ EdgeChunk edge_chunk (const uint8_t *__restrict__ seq, long n_bytes, long g)
{
  u32 w[4] = {0, 0, 0, 0};
#pragma unroll
  for (int b = 0; b < 16; b++) w[b >> 2] |= stream_byte (seq, n_bytes, g + b) << (8 * (b & 3));
  EdgeChunk e = {w[0], w[1], w[2], w[3]};
  return e;
}

// `raw` is the LDS-DMA landing zone: next tile's bytes arrive there straight from HBM; slot c is read and refilled only
// by the lane that owns chunk c.  It must be a __shared__ variable of its own: the compiler orders every later LDS access
// that MAY alias an in-flight LDS-DMA behind vmcnt(0), and members of one struct all may alias -- as part of TileLds the
// "prefetch" was waited for at the first LDS instruction after its issue.
// Where the tiles of a launch come from.  list == nullptr: the stream cut into n_tiles pieces of TILE bytes, handed out in
// groups of TJ_TILE_GROUP.  Otherwise: the tiles the fast kernel (scan_fast_kernel) left to this one -- tile t of that
// kernel owns the tract starts in [t * fown, (t + 1) * fown); each is covered here by NSUB = ceil (fown / TILE) pieces,
// handed out two at a time (the list is short, or the stream is slow-path material anyway).
#define TJ_LIST_FOWN 16288               // = FK_OWN (static_assert below): tract starts per listed tile
struct TileSrc { const u32 *list; long fown; };

template <int BLOCK, int TILE, int CANDDIV, class Sink>
__device__ __forceinline__ void scan_tiles (const uint8_t *__restrict__ seq, long n_bytes, long n_tiles, int k, int mprime,
                                            TileLds<BLOCK, TILE, CANDDIV> &T, uint4 *raw, Sink &sink, DevCounters *ctr, FixEntry *fix, u32 fix_cap, int par,
                                            const TileSrc src = TileSrc {nullptr, 0})
{
  typedef TileLds<BLOCK, TILE, CANDDIV> G;
  const int tid = threadIdx.x;
  const u64 km = kmask (k);
  const u64 kbits = (1ull << k) - 1ull;                 // k <= 32
  const bool listed = src.list != nullptr;
  constexpr u32 nsub_listed = (u32) ((TJ_LIST_FOWN + TILE - 1) / TILE);    // (compile-time: no division per tile)
  const u32 nsub = listed ? nsub_listed : 1u;
  u32 *const work = listed ? &ctr->lc[par].work_slow : &ctr->lc[par].work;
  if (listed) n_tiles = (long) ctr->lc[par].n_slow * (long) nsub;
  // (a group is reserved while its predecessor's first tile is worked on and looked up during the predecessor's last
  // tile: with at least two tiles per group a workgroup barrier lies between the two.  A short list is handed out two
  // pieces at a time, for balance; a long one -- a stream full of N, say -- in groups like the whole stream.)
  const u32 tgroup = !listed ? (u32) TJ_TILE_GROUP : (n_tiles >= 8l * TJ_TILE_GROUP * (long) gridDim.x) ? (u32) TJ_TILE_GROUP : 2u;
  // first stream byte a work item owns, and how many (multiples of 16); the list entry of the piece looked at last is
  // kept (the pieces of one listed tile follow each other)
  u32 le_idx = 0xFFFFFFFFu; long le_val = 0;
  auto own_start = [&] (long w) -> long {
    if (!listed) return w * (long) TILE;
    const u32 li = (u32) w / nsub_listed;
    if (li != le_idx) { le_idx = li; le_val = (long) src.list[li] * (long) TJ_LIST_FOWN; }
    return le_val + (long) ((u32) w % nsub_listed) * TILE;
  };
  auto own_len = [&] (long w) -> int { return listed ? (int) min ((long) TILE, (long) TJ_LIST_FOWN - (long) ((u32) w % nsub_listed) * TILE) : TILE; };

  // Tiles are handed out dynamically in groups of TJ_TILE_GROUP (one global atomic per group): workgroups differ in
  // how many tracts their tiles hold, and a static split leaves the slow ones running alone at the end.
  if (tid == 0) {
    T.odd[0] = 0; T.odd[1] = 0; T.grp[0] = atomicAdd (work, tgroup);
    if (blockIdx.x == 0 && !listed) { ctr->lc[par ^ 1].n_fix = 0; ctr->lc[par ^ 1].work = 0; ctr->lc[par ^ 1].n_slow = 0; ctr->lc[par ^ 1].work_slow = 0; ctr->lc[par ^ 1].ticket = 0; }
  }
  lds_barrier ();
  long tile = (long) T.grp[0];
  long grp_end = tile + tgroup;
  u32 gpar = 0, it = 0;
  if (tile < n_tiles) {
    const long w0 = own_start (tile) - TJ_HL;
#pragma unroll
    for (int i = 0; i < G::NLOAD; i++) {
      const int c = tid + i * BLOCK;
      if (c < G::NCHUNK) {
        issue_chunk (seq, n_bytes, w0 + 16l * c, &raw[c - (tid & 63)]);
        if ((tid & 63) == 0) issue_chunk (seq, n_bytes, w0 + 16l * (c - 1), &raw[G::NCHUNK + (tid >> 6) + i * (BLOCK / 64)]);
      }
    }
  }

  while (tile < n_tiles) {
    if (tid == 0 && tile + tgroup == grp_end) T.grp[gpar ^ 1u] = atomicAdd (work, tgroup);  // first tile of a group: reserve the next
    const long g0 = own_start (tile) - TJ_HL;           // stream position of window byte 0 (may be negative)
    const int olen = own_len (tile);                    // tract starts in window positions [TJ_HL, TJ_HL + olen) belong to this tile

    // ---- phase 1: classify the prefetched chunks into LDS, then prefetch the next tile ------------------------
    const u32 tpar = it & 1u;
    if (tid == 0) { T.ncand = 0; T.odd[tpar ^ 1u] = 0; }
    if (tid < 4) { T.code[G::CODEW - 4 + tid] = 0; T.start[G::MASKW - 4 + tid] = 0; T.sent[G::MASKW - 4 + tid] = 0xFFFFFFFFu; T.inval[G::MASKW - 4 + tid] = 0; }
    const bool interior = (g0 >= 0) && (g0 + (long) G::WIN <= n_bytes);   // whole window inside the stream (uniform)
    asm volatile ("s_waitcnt vmcnt(0)" ::: "memory");   // this lane's chunks of the tile have landed in raw
#pragma unroll
    for (int i = 0; i < G::NLOAD; i++) {
      const int c = tid + i * BLOCK;
      if (c < G::NCHUNK) {
        uint4 v = raw[c];
        if (!interior) {
          const long g = g0 + 16l * c;
          if (!((g >= 0) && (g + 16 <= n_bytes))) {
            const EdgeChunk e = edge_chunk (seq, n_bytes, g);
            v.x = e.x; v.y = e.y; v.z = e.z; v.w = e.w;
          }
        }
        const u32 w[4] = {v.x, v.y, v.z, v.w};
        u32 code32 = 0, st16 = 0, se16 = 0, iv16 = 0, bad = 0;
        // The byte in front of the chunk is the last byte of the lane before (one DPP move); the wave's first lane
        // finds it in the extra chunk its wave loaded for the purpose.
        u32 prevw = (u32) __builtin_amdgcn_update_dpp (0, (int) v.w, 0x138, 0xF, 0xF, false);      // wave_shr:1
        if ((tid & 63) == 0) {
          prevw = raw[G::NCHUNK + (tid >> 6) + i * (BLOCK / 64)].w;
          if (!interior) prevw = stream_byte (seq, n_bytes, g0 + 16l * c - 1) << 24;
        }
        const u32 prev0 = prevw >> 24;
#pragma unroll
        for (int j = 0; j < 4; j += 2) {                // two words per byte of the start / delimiter planes
          u32 c8a, c8b, s8 = 0, e8 = 0, ba, bb;
          classify_word_fast (w[j], prevw, false, c8a, s8, e8, ba);
          classify_word_fast (w[j + 1], w[j], true, c8b, s8, e8, bb);
          code32 |= (c8a | (c8b << 8)) << (16 * (j / 2));
          st16 |= j ? s8 << 1 : s8 >> 7;                // (s8 = 128 x the byte of 8 flags)
          se16 |= e8 << (4 * j); bad |= ba | bb;
          prevw = w[j + 1];
        }
        if (__builtin_expect (bad != 0u, 0)) {          // lower case, U, N, anything else: exact classification
          T.odd[tpar] = 1u;
          u32 prev = prev0;
          code32 = st16 = se16 = iv16 = 0;
          for (int j = 0; j < 4; j++) {
            u32 c8, s4, e4, i4;
            classify_word (w[j], prev, c8, s4, e4, i4);
            code32 |= c8 << (8 * j); st16 |= s4 << (4 * j); se16 |= e4 << (4 * j); iv16 |= i4 << (4 * j);
            prev = w[j] >> 24;
          }
        }
        T.code[c] = code32;
        reinterpret_cast<unsigned short *> (T.start)[c] = (unsigned short) st16;
        reinterpret_cast<unsigned short *> (T.sent)[c] = (unsigned short) se16;
        reinterpret_cast<unsigned short *> (T.inval)[c] = (unsigned short) (iv16 | se16);
      }
    }
    sink.tick ();
    // the tile after this one: the next of the group, or the first of the next group (reserved TJ_TILE_GROUP - 1 tiles ago)
    const long nt = (tile + 1 < grp_end) ? tile + 1 : (long) T.grp[gpar ^ 1u];
    {
      if (nt < n_tiles) {
        const long ng0 = own_start (nt) - TJ_HL;
        if (ng0 >= 16 && ng0 + (long) G::WIN <= n_bytes) {      // (uniform) the whole window and the chunk in front are inside: no per-lane checks
          const uint8_t *pl = seq + ng0 + 16l * tid;
#pragma unroll
          for (int i = 0; i < G::NLOAD; i++) {
            const int c = tid + i * BLOCK;
            if (c < G::NCHUNK) {
              lds_dma16 (pl + 16l * i * BLOCK, &raw[c - (tid & 63)]);
              if ((tid & 63) == 0) lds_dma16 (pl + 16l * i * BLOCK - 16, &raw[G::NCHUNK + (tid >> 6) + i * (BLOCK / 64)]);
            }
          }
        }
        else {
#pragma unroll
          for (int i = 0; i < G::NLOAD; i++) {
            const int c = tid + i * BLOCK;
            if (c < G::NCHUNK) {
              issue_chunk (seq, n_bytes, ng0 + 16l * c, &raw[c - (tid & 63)]);
              if ((tid & 63) == 0) issue_chunk (seq, n_bytes, ng0 + 16l * (c - 1), &raw[G::NCHUNK + (tid >> 6) + i * (BLOCK / 64)]);
            }
          }
        }
      }
    }
    lds_barrier ();

    // ---- phase 2: candidate tract starts among this lane's 16 positions ------------------------------------
    {
      const int p0 = TJ_HL + 16 * tid;
      const u64 S = bits64 (T.start, p0);
      u32 cand = (u32) S & 0xFFFFu;
      if (mprime <= 0) cand &= (u32) (S >> 1);                      // monomer mode: the next position starts a run too
      for (int j = 1; j < mprime; j++) cand &= ~(u32) (S >> j);     // next m'-1 positions continue the run
      cand &= ~(u32) reinterpret_cast<unsigned short *> (T.sent)[p0 >> 4];  // a run of delimiters is not a tract
      if (16 * tid >= olen) cand = 0;                               // (a listed tile may own less than TILE positions)
      // one LDS atomic per wavefront (512 same-address atomics serialise): exclusive prefix of the lane counts
      const u32 n = (u32) __popc (cand);
      const u32 incl = wave_inclusive_scan (n);
      const u32 total = (u32) __builtin_amdgcn_readlane ((int) incl, 63);     // (a uniform operand keeps the compiler's atomic optimiser from looping over lanes)
      u32 wbase = 0;
      if ((tid & 63) == 63 && total) wbase = atomicAdd (&T.ncand, total);
      wbase = (u32) __builtin_amdgcn_readlane ((int) wbase, 63);
      u32 at = wbase + incl - n;
      // (never more than MAXCAND in a tile: a candidate takes m' >= 2 positions -- one in the monomer mode, where MAXCAND = TILE)
      while (cand) { int b = __ffs ((int) cand) - 1; cand &= cand - 1u; T.cand[at] = (unsigned short) (p0 + b); at++; }
    }
    lds_barrier ();

    // ---- phase 3: one lane per candidate --------------------------------------------------------------------
    const int ncand = min ((int) T.ncand, G::MAXCAND);
    const bool tile_odd = T.odd[tpar] != 0u;            // some byte of this tile needed the exact classification
    for (int cb0 = 0; cb0 < ncand; cb0 += BLOCK) {
      const int ci = cb0 + tid;
      bool have = false;
      u64 c0 = 0, c1 = 0, pos = 0;
      u32 base = 0, flag = 0, len10 = 0;
      if (ci < ncand) {
        const int s = T.cand[ci];
        const long gs = g0 + s;
        int e = -1;                                   // run end: first run start after s
        const u32 ns32 = bits32 (T.start, s + 1);     // (within 32 positions for all but the longest tracts)
        if (ns32) e = s + __ffs ((int) ns32) - 1;
        else {
          const u64 ns = bits64 (T.start, s + 1);
          if (ns) e = s + __ffsll ((long long) ns) - 1;
          else for (int p = s + 65; p < G::WIN; p += 64) {
            const u64 n2 = bits64 (T.start, p);
            if (n2) { e = p + __ffsll ((long long) n2) - 2; break; }
          }
        }
        const bool inval = tile_odd && ((T.inval[s >> 5] >> (s & 31)) & 1u);
        bool ok;
        long len;
        u64 left = 0, right = 0;
        u32 cb = 0, linv = 0, rinv = 0;
        if (e >= 0 && e + k < G::WIN) {               // everything needed is in LDS
          len = e - s + 1;
          if (Sink::K32 || k <= 16) {                 // k <= 16: flanks, masks and k-mers fit 32-bit arithmetic (uniform branch)
            const u32 kb32 = (1u << k) - 1u, km32 = (k >= 16) ? 0xFFFFFFFFu : (1u << (2 * k)) - 1u;
            ok = (((bits32 (T.sent, s - k) | bits32 (T.sent, e + 1)) & kb32) == 0u);
            if (ok && !inval) {
              u32 l32 = bits32 (T.code, 2 * (s - k)) & km32, r32 = bits32 (T.code, 2 * (e + 1)) & km32;
              cb = (T.code[s >> 4] >> (2 * (s & 15))) & 3u;
              if (cb < 2u) { c0 = l32; c1 = r32; base = cb; flag = 1u; }
              else {
                if (tile_odd) {
                  linv = bits32 (T.inval, s - k) & kb32; rinv = bits32 (T.inval, e + 1) & kb32;
                  if (linv | rinv) { l32 |= (u32) spread_pairs (linv); r32 |= (u32) spread_pairs (rinv); }
                }
                c0 = revcomp_k32 (r32, k); c1 = revcomp_k32 (l32, k); base = 3u - cb; flag = 2u;
              }
              len10 = (u32) len & 0x3FFu;
              pos = (u64) gs;
              have = true;
              ok = false;                             // (record complete: skip the generic tail below)
            }
          }
          else {
            ok = ((bits64 (T.sent, s - k) & kbits) == 0ull) && ((bits64 (T.sent, e + 1) & kbits) == 0ull);
            if (ok && !inval) {
              left = bits64 (T.code, 2 * (s - k)) & km;
              right = bits64 (T.code, 2 * (e + 1)) & km;
              cb = (T.code[s >> 4] >> (2 * (s & 15))) & 3u;
              if (cb >= 2u && tile_odd) { linv = (u32) (bits64 (T.inval, s - k) & kbits); rinv = (u32) (bits64 (T.inval, e + 1) & kbits); }
            }
          }
        }
        else {                                        // tract runs past the window: walk the stream (rare)
          const u32 b = stream_byte (seq, n_bytes, gs);
          long ge = gs;
          while (stream_byte (seq, n_bytes, ge + 1) == b) ge++;
          len = ge - gs + 1;
          ok = flanks_from_stream (seq, n_bytes, gs, ge, k, left, right, linv, rinv);
          cb = byte_code (b);
        }
        if (ok) {
          if (!inval) {
            canonicalise (left, right, linv, rinv, cb, k, c0, c1, base, flag);
            len10 = (u32) ((u64) len & 0x3FFull);     // 10-bit store of the reference (src/hopo_counter.h:39)
            pos = (u64) gs;
            have = true;
          }
          else {                                      // non-ACGTU run: context comes from the previous tract of the read
            u64 at = atomicAdd ((unsigned long long *) &ctr->lc[par].n_fix, 1ull);
            if (at < fix_cap) { fix[at].pos = gs; fix[at].len = len; }
            else ctr->fix_overflow = 1u;
          }
        }
      }
      sink.put (have, c0, c1, base, len10, flag, pos, (u32) min (ncand - cb0, BLOCK));
    }
    lds_barrier ();
    if (tile + 1 >= grp_end) { gpar ^= 1u; grp_end = nt + tgroup; }
    tile = nt;
    it++;
  }
}

// Non-ACGTU runs that qualify as tracts (reference: src/hopo_counter.c:246-248: add_kmer is called with whatever the
// previous tract of the same read left in context[], hopo_base_int and reverse_forward_flag).  Walks back through the
// read to the nearest earlier recorded tract of a valid base; false = there is none (undefined in the reference).
__device__ bool stale_context (const uint8_t *__restrict__ seq, long n_bytes, long gs, int k, int mprime,
                               u64 &c0, u64 &c1, u32 &base, u32 &flag)
{
  long p = gs - 1;
  while (p >= 0 && seq[p] != '\n') {
    const u32 b = seq[p];
    long q = p;
    while (q - 1 >= 0 && seq[q - 1] == b) q--;          // run [q, p]
    // a recorded tract: >= m' equal bases -- or, in monomer mode (mprime <= 0), exactly one
    if (byte_is_acgtu (b) && (mprime > 0 ? (p - q + 1) >= mprime : p == q)) {
      u64 left, right; u32 linv, rinv;
      // recorded iff k bases of the same read precede it (its right side is fine: it ends before our run does);
      // an earlier run would start even closer to the read start, so the search stops here either way
      if (!flanks_from_stream (seq, n_bytes, q, p, k, left, right, linv, rinv)) return false;
      canonicalise (left, right, linv, rinv, byte_code (b), k, c0, c1, base, flag);
      return true;
    }
    p = q - 1;
  }
  return false;
}

// ---- sink 1: one list of located records (CPU-entry and test aid; small inputs) ------------------------------------

struct ListSink
{
  static constexpr bool K32 = false;
  u64 *out; u64 cap; DevCounters *ctr;
  __device__ __forceinline__ void tick () {}
  __device__ __forceinline__ void put (bool have, u64 c0, u64 c1, u32 base, u32 len10, u32 flag, u64 pos, u32 round_max)
  {
    emit_record<4> (have, c0, c1, make_meta (base, len10, flag), pos, out, cap, ctr);
  }
};

__global__ __launch_bounds__ (256)
void scan_list_kernel (const uint8_t *__restrict__ seq, long n_bytes, long n_tiles, int k, int mprime,
                       u64 *__restrict__ out, u64 cap, DevCounters *ctr, FixEntry *fix, u32 fix_cap, int par)
{
  __shared__ TileLds<256, 4096, 1> T;
  __shared__ uint4 raw[TileLds<256, 4096, 1>::NRAW];
  ListSink sink = {out, cap, ctr};
  scan_tiles<256, 4096, 1> (seq, n_bytes, n_tiles, k, mprime, T, raw, sink, ctr, fix, fix_cap, par);
}

__global__ void nrun_fixup_list_kernel (const uint8_t *__restrict__ seq, long n_bytes, int k, int mprime,
                                        u64 *__restrict__ out, u64 cap, DevCounters *ctr, const FixEntry *fix, u32 fix_cap, int par)
{
  u64 n_fix = ctr->lc[par].n_fix;
  if (n_fix > fix_cap) n_fix = fix_cap;
  for (u64 i = blockIdx.x * (u64) blockDim.x + threadIdx.x; i < n_fix; i += (u64) gridDim.x * blockDim.x) {
    u64 c0, c1; u32 base, flag;
    if (stale_context (seq, n_bytes, fix[i].pos, k, mprime, c0, c1, base, flag)) {
      u64 idx = atomicAdd (&ctr->n_rec, 1ull);
      if (idx < cap) store_record<4> (out, idx, c0, c1, make_meta (base, fix[i].len, flag), (u64) fix[i].pos);
      else ctr->overflow = 1u;
    }
    else atomicAdd (&ctr->n_undefined, 1ull);
  }
}

// ---- compact raw records and their hash ---------------------------------------------------------------------------
// Between the scan and the aggregation a raw tract is W 64-bit words, W chosen from k so that nothing is wasted:
//   W = 1 (k <= 12): low half  = ctx1 | len[7:0] << 24
//                    high half = ctx0 | len[9:8] << 24 | base << 26 | flag << 27      (fields at fixed places: packing is
//                    two shift-or instructions on 32-bit halves whatever k is; the word without its flag is the reduction key)
//   W = 2 (k <= 28): { 1 | base << 1 | len[4:0] << 2 | ctx0 << 7 ,  ctx1 | len[9:5] << 56 | flag << 61 }
//                    (word 0 is never 0 and never uses bit 63: the aggregation claims table slots with it)
//   W = 4          : { ctx0, ctx1, base | len << 2 | flag << 12, 0 }   (k > 28; padded so that 4 records fill a 128-byte line)
// flag == 3 never occurs in a raw record (one tract, one strand): it marks a padding ("null") record.

template <int W> __device__ __forceinline__ void pack_raw (u64 c0, u64 c1, u32 base, u32 len10, u32 flag, int k, u64 *w);
#define R1_FLAG_SHIFT 59                // W = 1 record: strand flag in bits 59-60 (27-28 of the high half)
#define R1_KEY_MASK   (~(3ull << R1_FLAG_SHIFT))
__device__ __forceinline__ u64 pack_rec1 (u32 c0, u32 c1, u32 base, u32 len10, u32 flag)
{
  const u32 lo = c1 | (len10 << 24), hi = c0 | ((len10 >> 8) << 24) | (base << 26) | (flag << 27);
  return ((u64) hi << 32) | lo;
}
template <> __device__ __forceinline__ void pack_raw<1> (u64 c0, u64 c1, u32 base, u32 len10, u32 flag, int k, u64 *w)
{ w[0] = pack_rec1 ((u32) c0, (u32) c1, base, len10, flag); }
template <> __device__ __forceinline__ void pack_raw<2> (u64 c0, u64 c1, u32 base, u32 len10, u32 flag, int k, u64 *w)
{ w[0] = 1ull | ((u64) base << 1) | ((u64) (len10 & 31u) << 2) | (c0 << 7); w[1] = c1 | ((u64) (len10 >> 5) << 56) | ((u64) flag << 61); }
template <> __device__ __forceinline__ void pack_raw<4> (u64 c0, u64 c1, u32 base, u32 len10, u32 flag, int k, u64 *w)
{ w[0] = c0; w[1] = c1; w[2] = (u64) base | ((u64) len10 << 2) | ((u64) flag << 12); w[3] = 0; }
template <int W> __device__ __forceinline__ void pack_null (u64 *w) { pack_raw<W> (0, 0, 0, 0, 3u, 2, w); }

template <int W> __device__ __forceinline__ void unpack_raw (const u64 *w, int k, u64 &c0, u64 &c1, u32 &base, u32 &len10, u32 &flag);
template <> __device__ __forceinline__ void unpack_raw<1> (const u64 *w, int k, u64 &c0, u64 &c1, u32 &base, u32 &len10, u32 &flag)
{
  const u32 lo = (u32) w[0], hi = (u32) (w[0] >> 32);
  c1 = lo & 0xFFFFFFu; c0 = hi & 0xFFFFFFu; len10 = (lo >> 24) | (((hi >> 24) & 3u) << 8); base = (hi >> 26) & 1u; flag = (hi >> 27) & 3u;
}
template <> __device__ __forceinline__ void unpack_raw<2> (const u64 *w, int k, u64 &c0, u64 &c1, u32 &base, u32 &len10, u32 &flag)
{
  const u64 m56 = (1ull << 56) - 1ull;
  c0 = (w[0] >> 7) & m56; c1 = w[1] & m56;
  base = (u32) (w[0] >> 1) & 1u; len10 = ((u32) (w[0] >> 2) & 31u) | (((u32) (w[1] >> 56) & 31u) << 5); flag = (u32) (w[1] >> 61) & 3u;
}
template <> __device__ __forceinline__ void unpack_raw<4> (const u64 *w, int k, u64 &c0, u64 &c1, u32 &base, u32 &len10, u32 &flag)
{ c0 = w[0]; c1 = w[1]; base = (u32) (w[2] & 3ull); len10 = (u32) ((w[2] >> 2) & 0x3FFull); flag = (u32) ((w[2] >> 12) & 3ull); }

// hash of the reduction key (base, context, stored length): bits 0-7 pick the bucket, 8-19 the table slot, 32-63 the tag
__device__ __forceinline__ u64 hash_key (u64 c0, u64 c1, u32 base, u32 len10)
{ // 32-bit arithmetic only (64-bit multiplies cost several quarter-rate instructions each); the tag merely has to
  // differ from the slot bits: a tag collision costs a key comparison, never a wrong answer
  u32 a = (u32) c0 ^ __builtin_amdgcn_alignbit ((u32) (c0 >> 32), (u32) (c0 >> 32), 25) ^ __builtin_amdgcn_alignbit ((u32) c1, (u32) c1, 19)
          ^ __builtin_amdgcn_alignbit ((u32) (c1 >> 32), (u32) (c1 >> 32), 11) ^ ((base | (len10 << 2)) * 0x9E3779B1u);
  u32 h = a * 0x85EBCA6Bu;
  h ^= h >> 15; h *= 0xC2B2AE35u; h ^= h >> 16;
  const u32 tag = (a ^ (a >> 13)) * 0x27D4EB2Fu;
  return ((u64) tag << 32) | h;
}

// bucket of a key: byte-wise dot products (full-rate v_dot4_u32_u8) instead of multiplies; the flank k-mers are close to
// uniform, so a weighted byte sum spreads them evenly enough over 256 buckets (the tables inside a bucket use hash_key)
__device__ __forceinline__ u32 bucket_of_key (u64 c0, u64 c1, u32 base, u32 len10)
{
  u32 h = __builtin_amdgcn_udot4 ((u32) c0, 0x6D2B4F0Bu, base | (len10 << 2), false);
  h = __builtin_amdgcn_udot4 ((u32) (c0 >> 32), 0x1D59A735u, h, false);
  h = __builtin_amdgcn_udot4 ((u32) c1, 0xC5A34D17u, h, false);
  h = __builtin_amdgcn_udot4 ((u32) (c1 >> 32), 0x3B7F9165u, h, false);
  return (h ^ (h >> 8)) & 255u;
}

// bucket of a one-word record (k <= 12), straight from its two halves (the strand flag is not part of the key)
__device__ __forceinline__ u32 bucket_of_rec1 (u32 lo, u32 hi)
{
  u32 h = __builtin_amdgcn_udot4 (lo, 0x6D2B4F0Bu, 0u, false);
  h = __builtin_amdgcn_udot4 (hi & 0x07FFFFFFu, 0xC5A34D17u, h, false);
  return (h ^ (h >> 8)) & 255u;
}

#define TJ_P        256                 // hash buckets
#define TJ_PBITS    8
#define TJ_STAGE_WORDS 2048
// TJ_STAGE_WORDS: 64-bit words of one-word records a workgroup stages in LDS between partition passes (twice that in the fast kernel)
#define TJ_CH0      1536                // chunk size unit in records; chunks are TJ_CH0 << ch_shift with ch_shift >= 2
#define TJ_EMPTY    0xFFFFFFFFu
// The bucket cursors take every reservation of every workgroup (millions of atomic adds per launch): each lives on a
// 256-byte line of its own, so that they spread over the memory channels instead of queueing up at the one or two that
// a packed 1 KB array maps to.  cursors[TJ_P * TJ_CSTRIDE] = the next free chunk.
#define TJ_CSTRIDE  64

// Bucket storage.  A bucket is a sequence of records numbered by its cursor; a workgroup reserves a run of positions
// with one atomic add and record `pos` lives in the bucket's (pos / CH)-th chunk (runs are shorter than a chunk, so a
// run straddles at most one chunk boundary).  Chunks come from one pool: chunk 0 of every bucket is assigned by the
// host, and the thread whose reservation holds the FIRST record of chunk j takes chunk j + 1 from the pool and
// publishes it in the bucket's table -- a whole chunk before anybody needs it, so nobody waits in practice, nothing
// leaks, and a skewed hash distribution costs nothing: memory follows the data, not the fullest bucket.
struct Buckets
{
  u64 *pool;          // pool_chunks * CH * W words
  u32 *table;         // [TJ_P][maxj] chunk ids, TJ_EMPTY = not claimed yet
  u32 *cursors;       // records reserved per bucket b at [b * TJ_CSTRIDE]
  u32 *pool_next;     // next free chunk
  u32 pool_chunks, maxj, ch_shift;      // CH = TJ_CH0 << ch_shift
};

#define TJ_NOCHUNK  0xFFFFFFFEu         // published instead of a chunk id when the pool is exhausted
#define TJ_SPIN_MAX (1u << 20)

__device__ __forceinline__ u32 chunk_of_pos (const Buckets &B, u32 pos) { return (pos / TJ_CH0) >> B.ch_shift; }

// Called by whoever reserved records [p0, p0 + n) of bucket b (n smaller than a chunk): if the reservation holds the
// first record of chunk j, claim chunk j + 1 (chunk 0 is pre-assigned).
__device__ __forceinline__ void bucket_claim_ahead (const Buckets &B, u32 b, u32 p0, u32 n, DevCounters *ctr)
{
  const u32 j = chunk_of_pos (B, p0 + n - 1);
  if (((j * TJ_CH0) << B.ch_shift) < p0) return;        // chunk j was opened by an earlier reservation
  if (j + 1 >= B.maxj) { ctr->overflow = 1u; return; }
  const u32 mine = atomicAdd (B.pool_next, 1u);
  if (mine >= B.pool_chunks) ctr->overflow = 1u;
  __hip_atomic_store (B.table + (u64) b * B.maxj + j + 1, mine < B.pool_chunks ? mine : TJ_NOCHUNK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the same for a reservation of any length: every chunk whose first record lies in [p0, p0 + n) has its successor claimed
__device__ __forceinline__ void bucket_claim_ahead_range (const Buckets &B, u32 b, u32 p0, u32 n, DevCounters *ctr)
{
  const u32 ch = (u32) TJ_CH0 << B.ch_shift;
  for (u32 j = (p0 + ch - 1u) / ch; (u64) j * ch < (u64) p0 + n; j++) {
    if (j + 1 >= B.maxj) { ctr->overflow = 1u; return; }
    const u32 mine = atomicAdd (B.pool_next, 1u);
    if (mine >= B.pool_chunks) ctr->overflow = 1u;
    __hip_atomic_store (B.table + (u64) b * B.maxj + j + 1, mine < B.pool_chunks ? mine : TJ_NOCHUNK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// chunk id of the j-th chunk of bucket b (TJ_NOCHUNK if it has none).  wait = the entry may still be on its way from
// the thread that claims it (same launch): poll it, bounded.
__device__ __forceinline__ u32 bucket_chunk_id (const Buckets &B, u32 b, u32 j, bool wait, DevCounters *ctr)
{
  if (j >= B.maxj) return TJ_NOCHUNK;
  u32 *e = B.table + (u64) b * B.maxj + j;
  u32 ch = __hip_atomic_load (e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (wait) {
    for (u32 spins = 0; ch == TJ_EMPTY && spins < TJ_SPIN_MAX; spins++) {
      __builtin_amdgcn_s_sleep (4);
      ch = __hip_atomic_load (e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (ch == TJ_EMPTY && ctr) ctr->overflow = 2u;          // (2: waited in vain for a chunk id -- a liveness problem, not a full pool)
  }
  return ch >= TJ_NOCHUNK ? TJ_NOCHUNK : ch;
}

// index (in records) inside the pool of record `pos` of bucket b; ~0 if it has no storage
__device__ __forceinline__ u64 bucket_slot (const Buckets &B, u32 b, u32 pos, bool wait, DevCounters *ctr)
{
  const u32 j = chunk_of_pos (B, pos);
  const u32 ch = bucket_chunk_id (B, b, j, wait, ctr);
  if (ch == TJ_NOCHUNK) return ~0ull;
  return (((u64) ch * TJ_CH0) << B.ch_shift) + (pos - ((j * TJ_CH0) << B.ch_shift));
}

template <int W>
__device__ __forceinline__ void bucket_insert_slow (u64 c0, u64 c1, u32 base, u32 len10, u32 flag, int k, const Buckets &B, DevCounters *ctr)
{
  u64 w[W];
  pack_raw<W> (c0, c1, base, len10, flag, k, w);
  const u32 b = (W == 1) ? bucket_of_rec1 ((u32) w[0], (u32) (w[0] >> 32)) : bucket_of_key (c0, c1, base, len10);
  const u32 pos = atomicAdd (&B.cursors[b * TJ_CSTRIDE], 1u);
  bucket_claim_ahead (B, b, pos, 1u, ctr);
  const u64 at = bucket_slot (B, b, pos, true, ctr);
  if (at != ~0ull) { u64 *q = B.pool + at * W; for (int j = 0; j < W; j++) q[j] = w[j]; }
}

// ---- sink 2: hash-partition into TJ_P buckets, in bulk ---------------------------------------------------------------
// Tracts are appended to an LDS staging buffer as they are found (one LDS atomic per wavefront, no barrier).  When the
// next round might not fit, the workgroup partitions what it has staged with one counting sort: count per bucket, one
// global atomic per non-empty bucket to reserve a run, permute in place (through registers) into bucket order, and
// write every run out contiguously.  All the fixed costs of partitioning (barriers, reservations, chunk look-ups) are
// paid once per ~4096 records instead of once per tile.

template <int W, int BIG = 0>
struct StageLds
{
  // a staged record is WS words (the 4th word of a W = 4 record is padding and only exists in HBM); the two-word and
  // three-word formats get 21 KB instead of 16: fewer, fuller partition passes (their fixed cost is per pass), still three
  // workgroups per CU
  static constexpr int WS = (W == 4) ? 3 : W;
  // BIG = the fast kernel's sink (scan_fast_kernel, two workgroups per CU): 4096 words of records are staged at a time
  // (4096 one-word records -- twice the records per pass, runs twice as long -- or 2048 two-word ones: the fast kernel's
  // LDS budget is the same for every k), and every array has 64 spare entries so that partition_big can do without
  // per-record branches
  // BIG = 2: partition_log_kernel's (two workgroups per CU and nothing else in LDS): 8192 one-word records per pass
  static constexpr int WORDS = BIG == 2 ? 8192 : BIG ? TJ_STAGE_WORDS * 2 : (W == 1) ? TJ_STAGE_WORDS : 2688;
  static constexpr int S = WORDS / WS;                   // records
  static constexpr int SPARE = BIG ? 64 : 0;
  u64 rec[WORDS + SPARE * WS];                          // (BIG: slots S + lane take the writes of lanes without a record)
  alignas (16) u64 gbase[TJ_P];                         // pool index of the first record of the bucket's run (BIG: gbase + gbase2 = 256 entries of 16 bytes, see partition_pass)
  u64 gbase2[TJ_P];                                     // pool index of the part of the run that lies in the next chunk
  alignas (16) u32 hist[TJ_P + SPARE];                  // (BIG: entries TJ_P + lane are for the lanes without a record)
  alignas (16) u32 offs[TJ_P + SPARE];                               // start of the bucket's run in the sorted staging buffer
  u32 split[BIG == 2 ? 1 : TJ_P];                       // records of the run before the chunk boundary (BIG: not used, the threshold travels in gbase's entry)
  u32 wsum[TJ_P / 64];
  u32 n;
  unsigned char bin[S + SPARE];
};

typedef StageLds<1, true> StageLdsFast1;
static_assert (offsetof (StageLdsFast1, gbase2) == offsetof (StageLdsFast1, gbase) + sizeof (u64) * TJ_P, "gbase and gbase2 back to back");

template <int W, int BLOCK, int BIG = 0>
struct StageSink
{
  static constexpr bool K32 = (W == 1);                 // k <= 12: the scan may use 32-bit k-mer arithmetic
  static constexpr int S = StageLds<W, BIG>::S;
  static constexpr int WS = StageLds<W, BIG>::WS;
  static constexpr int R = (S + BLOCK - 1) / BLOCK;     // staged records per thread in a partition pass
  // The fast kernel's one-word sink partitions exactly PS records at a time whenever it holds that many (the usual case:
  // a pass is asked for when the next round of BLOCK candidates might not fit, i.e. with S - BLOCK .. S records staged):
  // every round of the pass is full, so it is compiled without the "does this round hold a record" scalar tests (some 130
  // scalar instructions per wave and pass) and without the per-slot "is there a record" selects; what is staged beyond PS
  // (fewer than BLOCK records) moves to the front for the next pass.  PS = 0: no such pass.
  static constexpr int PS = (BIG && S > BLOCK && (S - BLOCK) % BLOCK == 0) ? S - BLOCK : 0;
  StageLds<W, BIG> &L;
  Buckets B; DevCounters *ctr; int k;
  u32 bound;                                            // upper bound of the records staged (workgroup-uniform)
  u32 cur_j, cur_chunk;                                 // owner thread (tid < TJ_P): the chunk its bucket is being written to

  __device__ __forceinline__ void start ()
  {
    if (threadIdx.x == 0) L.n = 0;
    if (BIG && threadIdx.x < TJ_P) L.hist[threadIdx.x] = 0;   // (partition_big leaves the counts zeroed for the pass after it)
    bound = 0; cur_j = TJ_EMPTY; cur_chunk = TJ_NOCHUNK;
    lds_barrier ();
  }

  __device__ __forceinline__ void tick () {}

  // `round_max`: workgroup-uniform upper bound of the lanes that bring a record in this call
  __device__ __forceinline__ void put (bool have, u64 c0, u64 c1, u32 base, u32 len10, u32 flag, u64 pos, u32 round_max)
  {
    if (bound + round_max > (u32) S) bound = partition ();
    bound += round_max;
    if (have) {
      // (a uniform-address atomic under a divergent condition: the compiler's atomic optimiser makes it one LDS atomic
      // per wavefront plus a lane prefix -- and does it better than the hand-written ballot / shuffle version did)
      const u32 at = atomicAdd (&L.n, 1u);
      u64 w[W];
      pack_raw<W> (c0, c1, base, len10, flag, k, w);
#pragma unroll
      for (int j = 0; j < WS; j++) L.rec[at * WS + j] = w[j];
      L.bin[at] = (unsigned char) (W == 1 ? bucket_of_rec1 ((u32) w[0], (u32) (w[0] >> 32)) : bucket_of_key (c0, c1, base, len10));
    }
  }

  // a one-word record already packed (scan_fast_kernel); same contract as put
  __device__ __forceinline__ void put1 (bool have, u32 lo, u32 hi, u32 round_max)
  {
    if (bound + round_max > (u32) S) bound = partition ();
    bound += round_max;
    if (have) {
      const u32 at = atomicAdd (&L.n, 1u);
      L.rec[at * WS] = ((u64) hi << 32) | lo;             // (W == 1)
      L.bin[at] = (unsigned char) bucket_of_rec1 (lo, hi);
    }
  }

  // the same in two steps, so that the slot's atomic is in flight while the caller works the record out:
  // reserve1 (round_max) by everybody; then per wave: lds_add_issue (count_addr (), records of the wave, raw); ...;
  // at = lds_collect (raw) + rank in the wave; if (have) store1 (at, lo, hi);
  __device__ __forceinline__ void reserve1 (u32 round_max)
  {
    if (bound + round_max > (u32) S) bound = partition ();
    bound += round_max;
  }
  __device__ __forceinline__ u32 count_addr () const { return (u32) (size_t) (lptr_t) &L.n; }
  __device__ __forceinline__ void store1 (u32 at, u32 lo, u32 hi)
  {
    L.rec[at * WS] = ((u64) hi << 32) | lo;
    L.bin[at] = (unsigned char) bucket_of_rec1 (lo, hi);
  }
  // the same with the hash's weights in VGPRs (h0 = 0x6D2B4F0B, h1 = 0xC5A34D17, m27 = 0x07FFFFFF: see bucket_of_rec1) and no branch: a
  // lane without a record passes at = S + lane, a spare slot
  __device__ __forceinline__ void store1v (u32 at, u32 lo, u32 hi, u32 h0, u32 h1, u32 m27)
  {
    L.rec[at * WS] = ((u64) hi << 32) | lo;
    u32 h = __builtin_amdgcn_udot4 (lo, h0, 0u, false);
    h = __builtin_amdgcn_udot4 (hi & m27, h1, h, false);
    L.bin[at] = (unsigned char) (h ^ (h >> 8));
  }
  __device__ __forceinline__ void store_fields (u32 at, u64 c0, u64 c1, u32 base, u32 len10, u32 flag)
  {
    u64 w[W];
    pack_raw<W> (c0, c1, base, len10, flag, k, w);
#pragma unroll
    for (int j = 0; j < WS; j++) L.rec[at * WS + j] = w[j];
    L.bin[at] = (unsigned char) (W == 1 ? bucket_of_rec1 ((u32) w[0], (u32) (w[0] >> 32)) : bucket_of_key (c0, c1, base, len10));
  }

  // The partition of the fast kernel's sink (BIG), written without per-record branches: a lane whose slot holds no
  // record works on spare bucket TJ_P + lane and spare staging slot S + lane, which exist for that purpose, and only its
  // store to the pool is masked; rounds r with r * BLOCK >= n hold no record at all and are skipped by a scalar branch.
  // (A branch per record costs three scalar instructions and an exec round trip, and scalar instructions are as dear as
  // vector ones on this chip.)
  // returns the records that stay staged (workgroup-uniform)
  __device__ __forceinline__ u32 partition_big (const bool final_pass = false)
  {
    lds_barrier ();                                     // every append so far is in LDS
    const u32 n = (u32) __builtin_amdgcn_readfirstlane ((int) L.n);
    if constexpr (PS > 0) {
      // (fewer than PS records: the caller's bound had counted candidates that were not recorded -- the round it asked
      // room for fits, n + BLOCK <= S, and the exact count is what it gets back; only finish () empties a partial buffer,
      // so that the loop holds one copy of the pass, the one without tests)
      if (n >= (u32) PS || final_pass) return final_pass ? partition_pass<false> (n) : partition_pass<true> (n);
      lds_barrier ();                                   // (rare path; nobody appends before everybody has read n)
      return n;
    }
    else return partition_pass<false> (n);
  }

  // FULL: the pass takes exactly the first PS staged records (all RR rounds are full); otherwise all n of them
  template <bool FULL>
  __device__ __forceinline__ u32 partition_pass (const u32 n)
  {
    static_assert (!BIG || BLOCK == 2 * TJ_P, "two threads per bucket");
    constexpr int RR = FULL ? PS / BLOCK : R;
    constexpr int H = (RR < 4) ? RR : 4;                // records per thread whose LDS loads are in flight together (2 and 8: the same time)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane (tid >> 6);
    // (five barriers per pass: the bucket counts are zero already -- zeroed below for the next pass, the spare ones are
    // never looked at -- and each of the four waves that own buckets works out the whole prefix for itself)
    u64 w[RR][WS], wrem[WS];
    u32 rk[RR], bb[RR], brem = 0;
#pragma unroll
    for (int r = 0; r < RR; r++)                        // my records ...
      if (FULL || (u32) r * BLOCK < n) {
        const u32 i = (u32) tid + (u32) r * BLOCK;
        bb[r] = L.bin[i];
#pragma unroll
        for (int j = 0; j < WS; j++) w[r][j] = L.rec[i * WS + j];
      }
    if constexpr (FULL) {                               // (what is staged beyond PS: kept in registers until the buffer is free)
      brem = L.bin[(u32) PS + (u32) tid];
#pragma unroll
      for (int j = 0; j < WS; j++) wrem[j] = L.rec[((u32) PS + (u32) tid) * WS + j];
    }
#pragma unroll
    for (int r = 0; r < RR; r++)                        // ... and their rank inside their bucket
      if (FULL || (u32) r * BLOCK < n) {
        const u32 i = (u32) tid + (u32) r * BLOCK;
        if constexpr (!FULL) bb[r] = (i < n) ? bb[r] : (u32) (TJ_P + lane);
        rk[r] = atomicAdd (&L.hist[bb[r]], 1u);
      }
    lds_barrier ();
    if (tid == 0) L.n = FULL ? n - (u32) PS : 0u;       // (everybody has read it; the next appends come after the last barrier below)
    u32 cnt = 0, p0 = 0, off = 0;
    if (wave < TJ_P / 64) {
      // exclusive prefix of the 256 bucket counts, four per lane, in each of the waves 0..3 (no exchange between them);
      // the wave writes the quarter that holds its own buckets and reads its bucket's entry back
      const uint4 h4 = *reinterpret_cast<const uint4 *> (&L.hist[4 * lane]);
      const u32 tot = h4.x + h4.y + h4.z + h4.w;
      const u32 e0 = wave_inclusive_scan (tot) - tot;
      if ((lane >> 4) == wave) *reinterpret_cast<uint4 *> (&L.offs[4 * lane]) = make_uint4 (e0, e0 + h4.x, e0 + h4.x + h4.y, e0 + h4.x + h4.y + h4.z);
      cnt = L.hist[tid];
      off = L.offs[tid];
      // reserve the bucket's run: the global atomic's round trip runs under the LDS permutation below (its result is
      // first looked at after that)
      if (cnt) p0 = atomicAdd (&B.cursors[tid * TJ_CSTRIDE], cnt);
    }
    else if (!FULL && wave == TJ_P / 64) L.offs[tid] = (u32) S + (u32) lane;   // (the spare entries: rank 0 lands on staging slot S + lane)
    lds_barrier ();
    if (tid < TJ_P) L.hist[tid] = 0;                    // (for the next pass)
    {
      u32 dst[RR];
#pragma unroll
      for (int r = 0; r < RR; r++) if (FULL || (u32) r * BLOCK < n) dst[r] = L.offs[bb[r]];
#pragma unroll
      for (int r = 0; r < RR; r++)                      // in-place permutation into bucket order (records are in registers)
        if (FULL || (u32) r * BLOCK < n) {
          const u32 d = FULL ? dst[r] + rk[r] : dst[r] + ((bb[r] < (u32) TJ_P) ? rk[r] : 0u);
#pragma unroll
          for (int j = 0; j < WS; j++) L.rec[d * WS + j] = w[r][j];
          L.bin[d] = (unsigned char) bb[r];
        }
    }
    if (wave < TJ_P / 64) {                             // where the reserved run lives: byte addresses of "sorted slot 0" for both parts
      // (tried in round 3: the usual run -- inside the chunk its bucket was written to last time, opening no new one -- worked
      // out without a branch and the rest behind one wave-wide test: 1.5 M vector and 0.5 M scalar instructions MORE per
      // launch, 1 % slower; the exec regions below are cheaper than they look)
      u64 a1 = 0, a2 = 0;
      u32 thr = 0;
      if (cnt) {
        const u32 ch = (u32) TJ_CH0 << B.ch_shift;
        bucket_claim_ahead (B, (u32) tid, p0, cnt, ctr);
        const u32 j0 = chunk_of_pos (B, p0), j1 = chunk_of_pos (B, p0 + cnt - 1);
        if (j0 != cur_j) { cur_j = j0; cur_chunk = bucket_chunk_id (B, (u32) tid, j0, true, ctr); }
        if (cur_chunk != TJ_NOCHUNK) a1 = (u64) (size_t) (B.pool + ((u64) cur_chunk * ch + (p0 - j0 * ch)) * W) - (8ull * W) * off;
        thr = off + cnt;
        if (j1 != j0) {                                 // the run crosses into the next chunk
          thr = off + (j1 * ch - p0);
          cur_j = j1; cur_chunk = bucket_chunk_id (B, (u32) tid, j1, true, ctr);
          if (cur_chunk != TJ_NOCHUNK) a2 = (u64) (size_t) (B.pool + ((u64) cur_chunk * ch) * W) - (8ull * W) * thr;
        }
      }
      // one 16-byte entry per bucket, read with one LDS instruction per record in the copy-out: [a1 low | a1 high (16 bits:
      // device addresses have 48) + thr << 16 | a2]   (gbase and gbase2 lie back to back: 256 x 16 bytes)
      reinterpret_cast<uint4 *> (L.gbase)[tid] = make_uint4 ((u32) a1, (u32) (a1 >> 32) | (thr << 16), (u32) a2, (u32) (a2 >> 32));
    }
    // Everything this wave has asked global memory for so far (the cursor's atomic, chunk ids, the tile's prefetch) is waited
    // for HERE, with the compiler's own instruction, before the first store below: from now on nothing is in flight that
    // anybody waits for but stores -- otherwise the compiler, unsure on which path a chunk id was fetched, puts a vmcnt(0)
    // where the tile loop's paths meet, in the classification of every tile, and that one waits for the stores too.
    __builtin_amdgcn_s_waitcnt (0x0F70);                // vmcnt(0) alone
    lds_barrier ();
#pragma unroll
    for (int r0 = 0; r0 < RR; r0 += H)
      if (FULL || (u32) r0 * BLOCK < n) {
        u32 cb[H], cthr[H];
        u64 ca1[H], ca2[H], cw[H][WS];
#pragma unroll
        for (int h = 0; h < H; h++) if (r0 + h < RR) cb[h] = L.bin[(u32) tid + (u32) (r0 + h) * BLOCK];
#pragma unroll
        for (int h = 0; h < H; h++) if (r0 + h < RR) {
          const u32 i = (u32) tid + (u32) (r0 + h) * BLOCK;
          const u32 b = cb[h] & (u32) (TJ_P - 1);       // (slots past n hold stale bytes: any bucket will do, the store is masked)
          const uint4 e = reinterpret_cast<const uint4 *> (L.gbase)[b];
          cthr[h] = e.y >> 16; ca1[h] = ((u64) (e.y & 0xFFFFu) << 32) | e.x; ca2[h] = ((u64) e.w << 32) | e.z;
#pragma unroll
          for (int j = 0; j < WS; j++) cw[h][j] = L.rec[i * WS + j];
        }
#pragma unroll
        for (int h = 0; h < H; h++) if (r0 + h < RR) {  // sorted slot i -> its place in the bucket's run (coalesced per run)
          const u32 i = (u32) tid + (u32) (r0 + h) * BLOCK;
          const u64 a = (i < cthr[h]) ? ca1[h] : ca2[h];
          const bool st = (FULL || i < n) && a != 0ull;
          if (st) {
            // (a pointer into the global address space, said so: made from an integer it is a generic pointer to the compiler, the
            // stores become flat_store -- which counts in lgkmcnt as well, completes out of order, and makes every later
            // wait of the wave a full drain of both counters)
            typedef __attribute__((address_space(1))) u64 *gwords_t;
            gwords_t q = (gwords_t) (a + (8ull * W) * i);
#pragma unroll
            for (int j = 0; j < WS; j++) q[j] = cw[h][j];
            if (WS < W) q[W - 1] = 0;
          }
        }
      }
    lds_barrier ();                                     // the staging buffer is free again
    if constexpr (FULL) {
      // what was staged beyond PS opens the next pass's buffer (the appends that follow go to slots n - PS and up: no
      // slot is written from both sides)
      if ((u32) PS + (u32) tid < n) {
#pragma unroll
        for (int j = 0; j < WS; j++) L.rec[(u32) tid * WS + j] = wrem[j];
        L.bin[tid] = (unsigned char) brem;
      }
      return n - (u32) PS;
    }
    return 0u;
  }

  __device__ __forceinline__ u32 partition (const bool final_pass = false)
  {
    if constexpr (BIG) return partition_big (final_pass);
    // (scan_bins_kernel, 80 registers: one record at a time)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    lds_barrier ();                                     // every append so far is in LDS
    const u32 n = L.n;
    if (tid < TJ_P) L.hist[tid] = 0;
    lds_barrier ();
    if (tid == 0) L.n = 0;                              // (everybody has read it; the next appends come after the last barrier below)
    u64 w[R][WS];
    u32 rk[R], bb[R];
#pragma unroll
    for (int r = 0; r < R; r++) {                       // my records and their rank inside their bucket
      const u32 i = (u32) tid + (u32) r * BLOCK;
      bb[r] = TJ_EMPTY;
      if (i < n) {
        bb[r] = L.bin[i];
#pragma unroll
        for (int j = 0; j < WS; j++) w[r][j] = L.rec[i * WS + j];
        rk[r] = atomicAdd (&L.hist[bb[r]], 1u);
      }
    }
    lds_barrier ();
    u32 cnt = 0, incl = 0;
    if (tid < TJ_P) {                                   // exclusive prefix of the bucket counts (waves 0..3)
      cnt = L.hist[tid];
      incl = wave_inclusive_scan (cnt);
      if (lane == 63) L.wsum[wave] = incl;
    }
    lds_barrier ();
    u32 p0 = 0;
    if (tid < TJ_P) {
      u32 wbase = 0;
      for (int v = 0; v < wave; v++) wbase += L.wsum[v];
      L.offs[tid] = wbase + incl - cnt;
      // reserve the bucket's run: the global atomic's round trip runs under the LDS permutation below (its result is
      // first looked at after that)
      if (cnt) p0 = atomicAdd (&B.cursors[tid * TJ_CSTRIDE], cnt);
    }
    lds_barrier ();
#pragma unroll
    for (int r = 0; r < R; r++)                         // in-place permutation into bucket order (records are in registers)
      if (bb[r] != TJ_EMPTY) {
        const u32 d = L.offs[bb[r]] + rk[r];
#pragma unroll
        for (int j = 0; j < WS; j++) L.rec[d * WS + j] = w[r][j];
        L.bin[d] = (unsigned char) bb[r];
      }
    if (tid < TJ_P && cnt) {                            // where the reserved run lives
      const u32 ch = (u32) TJ_CH0 << B.ch_shift;
      bucket_claim_ahead (B, (u32) tid, p0, cnt, ctr);
      const u32 j0 = chunk_of_pos (B, p0), j1 = chunk_of_pos (B, p0 + cnt - 1);
      if (j0 != cur_j) { cur_j = j0; cur_chunk = bucket_chunk_id (B, (u32) tid, j0, true, ctr); }
      L.gbase[tid] = (cur_chunk == TJ_NOCHUNK) ? ~0ull : (u64) cur_chunk * ch + (p0 - j0 * ch);
      u32 sp = cnt;
      u64 g2 = ~0ull;
      if (j1 != j0) {                                   // the run crosses into the next chunk
        sp = j1 * ch - p0;
        cur_j = j1; cur_chunk = bucket_chunk_id (B, (u32) tid, j1, true, ctr);
        if (cur_chunk != TJ_NOCHUNK) g2 = (u64) cur_chunk * ch;
      }
      L.split[tid] = sp; L.gbase2[tid] = g2;
    }
    lds_barrier ();
#pragma unroll
    for (int r = 0; r < R; r++) {                       // sorted slot i -> its place in the bucket's run (coalesced per run)
      const u32 i = (u32) tid + (u32) r * BLOCK;
      if (i < n) {
        const u32 b = L.bin[i], o = i - L.offs[b], sp = L.split[b];
        const u64 g = (o < sp) ? L.gbase[b] : L.gbase2[b];
        if (g != ~0ull) {
          u64 *q = B.pool + (g + (o < sp ? o : o - sp)) * W;
#pragma unroll
          for (int j = 0; j < WS; j++) q[j] = L.rec[i * WS + j];
          if (WS < W) q[W - 1] = 0;
        }
      }
    }
    lds_barrier ();                                     // the staging buffer is free again
    return 0u;
  }

  __device__ __forceinline__ void finish () { partition (true); }
};

#define TJ_SB_BLOCK 512
#define TJ_SB_TILE  8192
#define TJ_SB_WG_PER_CU 3               // grid = 3 workgroups per CU: 2 are resident (65 KB of LDS each), the queued third evens out the tail

// the qualifying runs of a non-ACGTU byte that scan_tiles has listed: their context is the tract before them (reference
// src/hopo_counter.c:246-248).  Entries first, first + step, ...
template <int W>
__device__ __forceinline__ void nrun_fixup_entries (const uint8_t *__restrict__ seq, long n_bytes, int k, int mprime, Buckets BK, DevCounters *ctr,
                                                    const FixEntry *fix, u32 fix_cap, int par, u64 first, u64 step)
{
  u64 n_fix = __hip_atomic_load (&ctr->lc[par].n_fix, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (n_fix > fix_cap) n_fix = fix_cap;
  for (u64 i = first; i < n_fix; i += step) {
    u64 c0, c1; u32 base, flag;
    if (stale_context (seq, n_bytes, fix[i].pos, k, mprime, c0, c1, base, flag))
      bucket_insert_slow<W> (c0, c1, base, (u32) ((u64) fix[i].len & 0x3FFull), flag, k, BK, ctr);
    else atomicAdd (&ctr->n_undefined, 1ull);
  }
}

template <int W>
__global__ __launch_bounds__ (TJ_SB_BLOCK, 6)
void scan_bins_kernel (const uint8_t *__restrict__ seq, long n_bytes, long n_tiles, int k, int mprime,
                       Buckets BK, DevCounters *ctr, FixEntry *fix, u32 fix_cap, int par, TileSrc src)
{
  __shared__ TileLds<TJ_SB_BLOCK, TJ_SB_TILE> T;
  __shared__ uint4 raw[TileLds<TJ_SB_BLOCK, TJ_SB_TILE>::NRAW];
  __shared__ StageLds<W> SL;
  // (behind the fast kernel: nothing was left over -- the usual case -- or a handful of tiles: one workgroup per listed tile is
  // plenty, the others leave here instead of paying for a sink's start and finish and, below, a device-scope fence each: with
  // 24 tiles listed the launch took 120 us for its 768 fences)
  const u32 n_listed = src.list ? ctr->lc[par].n_slow : 0u;
  const u32 n_active = src.list ? min (n_listed, (u32) gridDim.x) : (u32) gridDim.x;
  if (src.list && blockIdx.x >= n_active) return;
  StageSink<W, TJ_SB_BLOCK> sink = {SL, BK, ctr, k, 0u, 0u, 0u};
  sink.start ();
  scan_tiles<TJ_SB_BLOCK, TJ_SB_TILE, 2> (seq, n_bytes, n_tiles, k, mprime, T, raw, sink, ctr, fix, fix_cap, par, src);
  sink.finish ();
  if (src.list) {
    // Behind the fast kernel the fix-up of the listed runs is this kernel's last act instead of a launch of its own (which
    // cost 4 us of stream time per scan for nothing: with no tile on the list, the usual case, every workgroup has left at
    // the top and there is nothing to fix up).  The workgroup that finishes last does it: everybody's entries are released
    // by a device-scope fence in front of the ticket and acquired by one behind it -- a path taken by streams with
    // lower case, IUPAC codes or countable runs of 'N', where a fence's price does not matter.
    __shared__ u32 s_last;
    __threadfence ();
    __syncthreads ();
    if (threadIdx.x == 0) s_last = (atomicAdd (&ctr->lc[par].ticket, 1u) == n_active - 1u) ? 1u : 0u;
    __syncthreads ();
    if (s_last) {
      __threadfence ();
      nrun_fixup_entries<W> (seq, n_bytes, k, mprime, BK, ctr, fix, fix_cap, par, threadIdx.x, blockDim.x);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Fast scan for the streams that make up almost all input: tiles whose bytes are all upper-case A C G T or the read
// delimiter.  Same results as scan_tiles (reference: src/hopo_counter.c:219-258,285-307); any tile it cannot vouch for --
// a window that touches the stream's ends, a byte outside the five, more candidates than its list holds -- goes on a
// list that scan_bins_kernel works through afterwards (TileSrc), so nothing here has to know about lower case, U, N,
// the stale-context rule or stream edges.
//
// What makes it fast is the instruction mix.  On gfx950 a wave-wide and / or / xor / add / sub / right shift / mov /
// v_bitop3 whose operands are VGPRs, inline constants or (VOP1/VOP2) literals issues every 2 cycles; everything else --
// any SGPR operand, left shifts, v_perm, v_dot4, v_alignbit, DPP, v_lshl_or, v_ffbl, compares -- takes 4
// (tools/ubench/valu_rate3.hip).  So masks live in VGPRs, boolean algebra goes through v_bitop3, and the 4-cycle
// instructions are kept for what only they can do (byte table look-ups, bit gathers, funnel shifts).
//
// Geometry: 512 lanes x 32 bytes = a 16 KiB window per tile; the first 32 bytes (>= max k) and the last 64 are halo, the
// 16288 between them are the tract starts the tile owns (a tract whose end + k leaves the window walks the stream in
// global memory, like scan_tiles does).  A byte is one of the five iff the table look-up on its low three bits (all
// different: A 1, '\n' 2, C 3, T 4, G 7) gives the byte back; those three bits are then all that run detection needs
// (equal bytes <=> equal low bits), and code / letter / run-start bits are gathered with one v_dot4 per word each.
// Each lane keeps the run-start and letter masks of its 32 positions in registers and finds its candidates from them
// (plus one DPP move for the next lane's bits); the rest is scan_tiles' phase 3 with 32-bit windows: one funnel read of
// the run-start plane for the run end, one of the letter plane for "k letters on both sides" (whenever 2k + length <= 32),
// one of the code plane per flank.

// ---- sink 3: the record log (one-word records: k <= 12) ---------------------------------------------------------------
// scan_fast_kernel<1> does not partition: a recorded tract goes straight from the lane that worked it out to the next
// free word of a linear log -- blocks of TJ_LOGB records that a workgroup takes from a counter one ahead of need (the
// atomic's result is picked up a tile later), slot = the workgroup's running count (one LDS atomic per wave and round, as
// the staging buffer's was).  partition_log_kernel then reads the log back at memory speed and distributes it over the
// hash buckets with the counting sort of StageSink::partition_pass -- a kernel of its own with six waves per SIMD, in
// which that sort's barriers and atomic round trips hide behind other workgroups, instead of a pass that stalls a
// scanning workgroup 32 times per launch with 37 KB of its LDS and 45 of its registers set aside for it.
#define TJ_LOGB_SHIFT 13
#define TJ_LOGB       (1u << TJ_LOGB_SHIFT)             // records per log block (a tile brings at most FK_MAXCAND = 4096)
#define TJ_LOG_AHEAD  (2u * 4096u + 1024u)              // a block is asked for when the count may reach it within two tiles
struct LogSpace
{
  u64 *log;             // n_blocks * TJ_LOGB records, then 64 scratch words per workgroup of the scan
  u32 *next;            // blocks handed out
  u32 *next_other;      // the next launch's counter (launches alternate between two): zeroed by this launch
  u32 *count;           // [n_blocks] records in each block (written by the workgroup that filled it)
  u32 n_blocks;
};

struct LogLds
{
  alignas (16) u64 blk[4];              // byte address of the block that holds the workgroup's records j * TJ_LOGB ..., j & 3
  u32 id[4];
  u32 n;                                // records appended by this workgroup
};

// W: words per record (1: k <= 12, 2: k <= 28).  A block is TJ_LOGB words whatever W is: 8192 one-word or 4096 two-word records.
template <int W>
struct LogSink
{
  static_assert (W == 1 || W == 2, "the log holds one-word and two-word records");
  static constexpr int S = 0x7FFFFFF0;                  // (no buffer to fill up: every tile "fits")
  static constexpr u32 RS = TJ_LOGB_SHIFT - (W == 2 ? 1 : 0), RB = 1u << RS;     // records per block
  LogLds &L;
  LogSpace G; DevCounters *ctr; int k;
  u32 bound;
  u32 upto, pend, pend_id;                              // thread 0: last block index with an address in L.blk; a reservation on its way
  u64 scratch;                                          // where lanes without a record write (byte address, 64 words per workgroup)

  __device__ __forceinline__ u64 block_addr (u32 id) const
  {
    // (cannot happen: the log is sized for a tract every m' bytes.  If it did: the flag makes the scan fail; until then the
    // records go to block 0, inside the log -- the scratch words are 64 per workgroup, not a block)
    if (id >= G.n_blocks) { ctr->overflow = 1u; return (u64) (size_t) G.log; }
    return (u64) (size_t) G.log + (((u64) id << TJ_LOGB_SHIFT) << 3);
  }
  __device__ __forceinline__ void start ()
  {
    bound = 0; pend = 0; pend_id = 0; upto = 1;
    scratch = (u64) (size_t) G.log + ((((u64) G.n_blocks << TJ_LOGB_SHIFT) + 64ull * blockIdx.x) << 3);
    if (threadIdx.x == 0) {
      L.n = 0;
      const u32 b0 = atomicAdd (G.next, 2u);
      L.id[0] = b0; L.id[1] = b0 + 1u; L.id[2] = ~0u; L.id[3] = ~0u;
      L.blk[0] = block_addr (b0); L.blk[1] = block_addr (b0 + 1u); L.blk[2] = scratch; L.blk[3] = scratch;
    }
    lds_barrier ();
  }
  // top of a tile, every outstanding load of the wave waited for: a block that was asked for a tile ago has its address now
  // (the ring slot it takes held block upto - 3, which is full -- or will be when the kernel ends: slots are handed out densely)
  __device__ __forceinline__ void collect ()
  {
    if (threadIdx.x == 0 && pend) {
      upto++;
      const u32 slot = upto & 3u, old = L.id[slot];
      if (old < G.n_blocks) G.count[old] = RB;
      L.id[slot] = pend_id; L.blk[slot] = block_addr (pend_id);
      pend = 0;
    }
  }
  // `n`: the workgroup's count, read while nobody appends.  (A tile brings at most FK_MAXCAND = 4096 records, a block
  // holds at least as many: at most one new block per tile, asked for TJ_LOG_AHEAD records -- two tiles -- ahead, so that the
  // tile after the asking one, which picks the address up at its top, is the first that can need it; the ring slot it
  // takes held block j - 4 while the appends are at j - 3 or later.)
  __device__ __forceinline__ void tile_top (u32 n)
  {
    if (threadIdx.x == 0 && !pend && ((n + TJ_LOG_AHEAD) >> RS) > upto) { pend_id = atomicAdd (G.next, 1u); pend = 1u; }
  }
  __device__ __forceinline__ void reserve1 (u32) {}
  __device__ __forceinline__ u32 count_addr () const { return (u32) (size_t) (lptr_t) &L.n; }
  __device__ __forceinline__ u64 place (u32 at) const { return L.blk[(at >> RS) & 3u] + (8ull * W) * (at & (RB - 1u)); }
  __device__ __forceinline__ void store1 (u32 at, u32 lo, u32 hi)
  {
    typedef __attribute__((address_space(1))) u64 *gwords_t;
    *(gwords_t) place (at) = ((u64) hi << 32) | lo;
  }
  // branch-free: a lane without a record writes to the workgroup's scratch words
  __device__ __forceinline__ void store1ok (bool ok, u32 at, u32 lo, u32 hi, u32 lane)
  {
    typedef __attribute__((address_space(1))) u64 *gwords_t;
    const u64 a = place (at);
    *(gwords_t) (ok ? a : scratch + 8ull * lane) = ((u64) hi << 32) | lo;
  }
  // a record from its fields (the two-word kernel's phase 3)
  __device__ __forceinline__ void store_fields (u32 at, u64 c0, u64 c1, u32 base, u32 len10, u32 flag)
  {
    typedef __attribute__((address_space(1))) u64 *gwords_t;
    u64 w[W];
    pack_raw<W> (c0, c1, base, len10, flag, k, w);
    gwords_t q = (gwords_t) place (at);
#pragma unroll
    for (int j = 0; j < W; j++) q[j] = w[j];
  }
  __device__ __forceinline__ void finish ()
  {
    lds_barrier ();
    collect ();
    if (threadIdx.x == 0) {
      const u32 n = L.n;
      for (u32 j = (upto >= 3u ? upto - 3u : 0u); j <= upto; j++) {
        const u32 id = L.id[j & 3u];
        if (id < G.n_blocks) G.count[id] = (n > (j << RS)) ? min (n - (j << RS), RB) : 0u;
      }
    }
  }
};

#define FK_BLOCK    512
#define FK_WG_PER_CU 2
#define FK_LOG_WG_PER_CU 3              // the log variant (no staging buffer: 35 KB of LDS)
// FK_WG_PER_CU: 73 KB of LDS each (the 4096-record staging buffer is worth more than a third workgroup)
#define FK_UNIT     32                  // stream bytes per lane
#define FK_WIN      (FK_BLOCK * FK_UNIT)
#define FK_HL       32
#define FK_HR       64
#define FK_OWN      (FK_WIN - FK_HL - FK_HR)
static_assert (FK_OWN == TJ_LIST_FOWN, "scan_tiles' list mode is compiled for the fast kernel's tile size");
#define FK_MAXCAND  4096
// FK_MAXCAND: (a tile with more candidates goes to the generic kernel: more than one per 4 positions)
#define FK_GROUP    4                   // tiles per work-counter atomic (8: 1.5 % slower, a longer tail; 2: 5 % slower)

struct FastLds
{
  u32 code[FK_WIN / 16 + 4];            // 2-bit codes, 16 positions per word (+ zeroed pad for funnel reads)
  u32 st[FK_WIN / 32 + 4];              // run starts (byte differs from its predecessor)
  u32 lt[FK_WIN / 32 + 4];              // letters (not a read delimiter)
  unsigned short cand[FK_MAXCAND + 2 + 64];         // (+ 64: unused; the spare entry per lane of the tried variant of the candidate loop below -- kept so that the LDS layout stays as measured)
  u32 ncand[4];                         // per tile, three in rotation (zeroed two tiles ahead)
  u32 bad[4];                           // per tile, likewise: some byte outside ACGT\n
  u32 grp[2];
  u32 sbuf[32];                         // tiles given up, on their way to the slow list (one global atomic per 32)
  u32 np[FK_WIN / 32 + 4];              // second chance of a tile (see the kernel): positions that hold an 'N'
  u32 ncand2;                           // its candidate count
};

// v_bitop3_b32 truth tables: bit (a << 2 | b << 1 | c) of the immediate = f (a, b, c)
#define BITOP3_XOR_AND   0x48           // (a ^ c) & b
#define BITOP3_OR_XOR    0xF6           // a | (b ^ c)

// reverse complement of a k-mer of at most 16 bases with the constants in VGPRs: bit reverse, then swap the two bits of
// every base and complement in one v_bitop3 (rs = 32 - 2k)
__device__ __forceinline__ u32 revcomp_v32 (u32 x, u32 m55, u32 rs)
{
  const u32 y = __brev (x);
  // ~(((y >> 1) & 0x5555...) | ((y << 1) & 0xAAAA...)): a = y >> 1, b = y + y, c = mask -> ~(c ? a : b)
  const u32 z = __builtin_amdgcn_bitop3_b32 (y >> 1, y + y, m55, 0x1B);
  return z >> rs;
}

// Phase 3 of scan_fast_kernel for any k: run end from the run-start plane (32 positions first, then 64-bit windows), the
// two flanks checked against the letter plane and pulled out of the code plane separately (32-bit arithmetic for
// k <= 16), and past the window's end a walk through the stream in global memory -- scan_tiles' logic on this kernel's
// planes.  Returns false if the tract is not recorded.
template <bool K32>
__device__ __forceinline__ bool fast_tract (const FastLds &T, const uint8_t *__restrict__ seq, long n_bytes, long g0, int s, int k, int mprime,
                                            u64 &c0, u64 &c1, u32 &base, u32 &len10, u32 &flag, bool n_tile = false)
{
  int e = -1;
  {
    const u32 ns32 = bits32 (T.st, s + 1);
    if (ns32) e = s + __ffs ((int) ns32) - 1;
    else {
      const u64 ns = bits64 (T.st, s + 1);
      if (ns) e = s + __ffsll ((long long) ns) - 1;
      else for (int p = s + 65; p < FK_WIN; p += 64) {
        const u64 n2 = bits64 (T.st, p);
        if (n2) { e = p + __ffsll ((long long) n2) - 2; break; }
      }
    }
  }
  const long gs = g0 + s;
  long len;
  if (e >= 0 && e + k < FK_WIN) {                       // everything needed is in LDS
    len = e - s + 1;
    const u32 kb32 = (k >= 32) ? 0xFFFFFFFFu : (1u << k) - 1u;
    if ((((~bits32 (T.lt, s - k) | ~bits32 (T.lt, e + 1)) & kb32) != 0u) || len < mprime) return false;
    const u32 cb = (T.code[s >> 4] >> (2 * (s & 15))) & 3u;
    // (a tile with 'N's: an 'N' in a flank has code 0 in the plane, which is what the reference packs for it read forwards;
    // read backwards it packs 0 as well, not the complement -- its forward code is made 3 before complementing, as
    // `canonicalise` does for every non-ACGTU byte)
    u64 nl2 = 0, nr2 = 0;
    if (n_tile) {
      const u32 nl = bits32 (T.np, s - k) & kb32, nr = bits32 (T.np, e + 1) & kb32;
      if (nl | nr) { nl2 = spread_pairs (nl); nr2 = spread_pairs (nr); }
    }
    if (K32 || k <= 16) {
      const u32 km32 = (k >= 16) ? 0xFFFFFFFFu : (1u << (2 * k)) - 1u;
      const u32 l32 = bits32 (T.code, 2 * (s - k)) & km32, r32 = bits32 (T.code, 2 * (e + 1)) & km32;
      if (cb < 2u) { c0 = l32; c1 = r32; base = cb; flag = 1u; }
      else { c0 = revcomp_k32 (r32 | (u32) nr2, k); c1 = revcomp_k32 (l32 | (u32) nl2, k); base = 3u - cb; flag = 2u; }
    }
    else {
      const u64 km = kmask (k);
      const u64 left = bits64 (T.code, 2 * (s - k)) & km, right = bits64 (T.code, 2 * (e + 1)) & km;
      if (cb < 2u) { c0 = left; c1 = right; base = cb; flag = 1u; }
      else { c0 = revcomp_k (right | nr2, k); c1 = revcomp_k (left | nl2, k); base = 3u - cb; flag = 2u; }
    }
  }
  else {                                                // the tract runs past the window: walk the stream (rare)
    const u32 b = stream_byte (seq, n_bytes, gs);
    long ge = gs;
    while (stream_byte (seq, n_bytes, ge + 1) == b) ge++;
    len = ge - gs + 1;
    u64 left, right; u32 linv, rinv;
    // (outside the window bytes may be anything: non-ACGTU flank bases pack as 0 in both orientations)
    if (!flanks_from_stream (seq, n_bytes, gs, ge, k, left, right, linv, rinv) || len < mprime) return false;
    canonicalise (left, right, linv, rinv, byte_code (b), k, c0, c1, base, flag);
  }
  len10 = (u32) ((u64) len & 0x3FFull);
  return true;
}

// the same, out of line, for the tracts that do not fit the one-word kernel's straight-line path (k + length + k > 32).
// Returns the packed record, 0 if the tract is not recorded (a record is never 0; by value: a reference parameter of a
// function that is not inlined would put the caller's variables into scratch memory, in every round).
__device__ __noinline__ u64 fast_general_tract (const FastLds &T, const uint8_t *__restrict__ seq, long n_bytes, long g0, int s, int k, int mprime, bool n_tile)
{
  u64 c0, c1; u32 base, len10, flag;
  if (!fast_tract<true> (T, seq, n_bytes, g0, s, k, mprime, c0, c1, base, len10, flag, n_tile)) return 0ull;
  return pack_rec1 ((u32) c0, (u32) c1, base, len10, flag);
}

// two LDS-DMA loads of 1 KiB each (lane l: 16 bytes at sbase + voff, voff = 16 l) with a wave-uniform base address in
// SGPRs and one M0 write: the instruction offset of the second load moves its global address and its LDS address alike
__device__ __forceinline__ void lds_dma32 (const uint8_t *sbase, u32 voff, void *lds_wave_base)
{
  const u32 m0v = (u32) (size_t) (lptr_t) lds_wave_base;
  // (M0 is the compiler's: as an operand bound to that register it writes it itself, one s_mov, and knows that it did)
  asm volatile ("s_nop 0\n\tglobal_load_lds_dwordx4 %0, %1\n\tglobal_load_lds_dwordx4 %0, %1 offset:1024"
                :: "v"(voff), "s"(sbase), "{m0}"(m0v) : "memory");
}

// (88 scalar registers at most.  A SIMD hands out its 800 in blocks of 16, plus 16 per wavefront: the log variant took 106,
// six wavefronts of 112 + 16 left 32, and no kernel could start beside it although registers, wavefront slots and LDS were
// there -- the ordering step of the sample before, queued on the side stream, waited for the scan's end.  At 86 (ten more
// values kept in lanes of a vector register) six wavefronts take 672 and leave 128: a guest of up to 112.  The variants that
// partition by themselves are bounded to four wavefronts per SIMD and keep their 106; tests/test_order_budget.py)
template <int W, bool LOG = false>
__global__ __launch_bounds__ (FK_BLOCK, FK_BLOCK * (LOG ? FK_LOG_WG_PER_CU : FK_WG_PER_CU) / 256) __attribute__ ((amdgpu_num_sgpr (88)))
void scan_fast_kernel (const uint8_t *__restrict__ seq, long n_bytes, long n_ftiles, int k, int mprime,
                       Buckets BK, DevCounters *ctr, u32 *__restrict__ slow_list, int par, int all_slow, LogSpace LG)
{
  static_assert (!LOG || W <= 2, "the record log holds one-word and two-word records");
  __shared__ FastLds T;
  __shared__ uint4 raw[FK_WIN / 16];
  __shared__ std::conditional_t<LOG, LogLds, StageLds<W, true>> SL;
  auto make_sink = [&] () {
    if constexpr (LOG) return LogSink<W> {SL, LG, ctr, k, 0u, 0u, 0u, 0u, 0ull};
    else return StageSink<W, FK_BLOCK, true> {SL, BK, ctr, k, 0u, 0u, 0u};
  };
  auto sink = make_sink ();
  sink.start ();

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane (tid >> 6);
  // masks in VGPRs (an SGPR or literal operand would halve the issue rate of the instructions that use them)
  u32 M07, M06, M40;
  asm ("v_mov_b32 %0, 0x07070707" : "=v"(M07));
  asm ("v_mov_b32 %0, 0x06060606" : "=v"(M06));
  asm ("v_mov_b32 %0, 0x40404040" : "=v"(M40));
  u32 M55, vk, vk2, vkm, vrs, v32, vmp;                 // likewise the uniform values that phase 3 combines with per-lane data
  asm ("v_mov_b32 %0, 0x55555555" : "=v"(M55));
  asm ("v_mov_b32 %0, %1" : "=v"(vk) : "s"(k));
  asm ("v_mov_b32 %0, %1" : "=v"(vk2) : "s"(2 * k));
  asm ("v_mov_b32 %0, %1" : "=v"(vkm) : "s"(W == 1 ? (1u << (2 * k)) - 1u : 0u));     // (the straight-line phase 3 is for k <= 12)
  asm ("v_mov_b32 %0, %1" : "=v"(vrs) : "s"(W == 1 ? 32 - 2 * k : 0));
  asm ("v_mov_b32 %0, 32" : "=v"(v32));
  asm ("v_mov_b32 %0, %1" : "=v"(vmp) : "s"(mprime));
  u32 vm3, vm4, vh0, vh1, vm27;                             // "mprime >= 3", "mprime >= 4" as masks; the bucket hash's weights
  asm ("v_mov_b32 %0, %1" : "=v"(vm3) : "s"(mprime >= 3 ? 0xFFFFFFFFu : 0u));
  asm ("v_mov_b32 %0, %1" : "=v"(vm4) : "s"(mprime >= 4 ? 0xFFFFFFFFu : 0u));
  asm ("v_mov_b32 %0, 0x6D2B4F0B" : "=v"(vh0));
  asm ("v_mov_b32 %0, 0xC5A34D17" : "=v"(vh1));
  asm ("v_mov_b32 %0, 0x07FFFFFF" : "=v"(vm27));
  u32 own = (tid == 0 || tid >= (FK_WIN - FK_HR) / FK_UNIT) ? 0u : 0xFFFFFFFFu;   // halo lanes own no tract start
  asm volatile ("" : "+v"(own));                        // (a VGPR, not a condition that is looked up in spilled SGPRs per tile)
  const u32 voff16 = 16u * (u32) lane;

  // Scalar instructions are not free on this chip (about 4.6 cycles each per SIMD, tools/ubench/valu_salu.hip), so the
  // loop's bookkeeping is kept to 32-bit scalars: a launch covers less than 2 GiB (scan_device_piece), tile numbers and
  // byte offsets fit an int.  Tiles 1 .. t_hi have their whole window (and the 16 bytes in front) inside the stream.
  const int nt_all = (int) n_ftiles, nb = (int) n_bytes;
  const int t_hi = (nb >= FK_WIN - FK_HL) ? (nb - (FK_WIN - FK_HL)) / FK_OWN : 0;
  if (all_slow) {                                       // (tests: every tile goes to the generic kernel)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      for (int t = 0; t < nt_all; t++) slow_list[t] = (u32) t;
      ctr->lc[par].n_slow = (u32) nt_all; ctr->lc[par].work = (u32) nt_all;
      ctr->lc[par ^ 1].n_fix = 0; ctr->lc[par ^ 1].work = 0; ctr->lc[par ^ 1].n_slow = 0; ctr->lc[par ^ 1].work_slow = 0; ctr->lc[par ^ 1].ticket = 0;
      if constexpr (LOG) *LG.next_other = 0u;
    }
    sink.finish ();
    return;
  }
  const u32 ncand_addr = (u32) (size_t) (lptr_t) &T.ncand[0];

  if (wave == 0) {
    if (lane == 0) {
      T.grp[0] = atomicAdd (&ctr->lc[par].work, (u32) FK_GROUP);
      if (blockIdx.x == 0) {
        ctr->lc[par ^ 1].n_fix = 0; ctr->lc[par ^ 1].work = 0; ctr->lc[par ^ 1].n_slow = 0; ctr->lc[par ^ 1].work_slow = 0; ctr->lc[par ^ 1].ticket = 0;
        if constexpr (LOG) *LG.next_other = 0u;
      }
    }
    if (lane < 4) { T.ncand[lane] = 0; T.bad[lane] = 0; T.code[FK_WIN / 16 + lane] = 0; T.st[FK_WIN / 32 + lane] = 0; T.lt[FK_WIN / 32 + lane] = 0; T.np[FK_WIN / 32 + lane] = 0; T.ncand2 = 0; }
  }
  // (phase 3 reads the candidate list with a clamped index instead of a branch: every entry must be a position)
  for (int i = tid; i < FK_MAXCAND + 2; i += FK_BLOCK) T.cand[i] = (unsigned short) FK_HL;
  lds_barrier ();
  int tile = __builtin_amdgcn_readfirstlane ((int) T.grp[0]);
  int grp_end = tile + FK_GROUP;
  u32 gpar = 0, it = 0;

  // next tile's bytes: HBM -> LDS, 2 KiB per wave (two instructions of 1 KiB), and the word in front of the wave's
  // first byte.  The stream's first and last tiles are done here too: their chunks that stick out are fetched from a
  // valid address instead and phase 1 overwrites what lies outside the stream with read delimiters (edge_chunk).
  u32 pred = 0;
  // (the interior test comes first and stands for "there is such a tile" as well: tiles 1 .. t_hi all exist, so the usual
  // tile pays one compare, not two; its byte offset is non-negative and is added as an unsigned number)
  auto prefetch = [&] (int t) {
    const int g0w = t * FK_OWN - FK_HL + 2048 * wave;   // stream position of the wave's first byte
    if ((u32) (t - 1) < (u32) t_hi) {
      const uint8_t *g = seq + (u32) g0w;
      lds_dma32 (g, voff16, &raw[128 * wave]);
      pred = *reinterpret_cast<const u32 *> (g - 4);
    }
    else if (t < nt_all) {
      issue_chunk (seq, n_bytes, (long) g0w + 16l * lane, &raw[128 * wave]);
      issue_chunk (seq, n_bytes, (long) g0w + 1024l + 16l * lane, &raw[128 * wave + 64]);
      pred = stream_byte (seq, n_bytes, (long) g0w - 1) << 24;
    }
  };
  prefetch (tile);
  u32 n_sbuf = 0;                                       // (workgroup-uniform)
  auto flush_slow = [&] () {
    if (wave == 0 && n_sbuf) {                          // (thread 0 wrote the entries: same wave, LDS keeps its order)
      u32 base = 0;
      if (lane == 0) base = atomicAdd (&ctr->lc[par].n_slow, n_sbuf);
      base = (u32) __builtin_amdgcn_readfirstlane ((int) base);
      if ((u32) lane < n_sbuf) slow_list[base + (u32) lane] = T.sbuf[lane];
    }
    n_sbuf = 0;
  };

  while (tile < nt_all) {
    const u32 slot = it & 3u;
    // (opaque: as a loop invariant the compiler keeps "wave == 0" as a 64-bit mask in a spilled pair of SGPRs and pays two
    // v_readlane and an s_and per tile to look at it; compared afresh it is one s_cmp)
    int wave_now = wave;
    asm volatile ("" : "+s"(wave_now));
    if (wave_now == 0) {
      if (tile + FK_GROUP == grp_end) { if (lane == 0) T.grp[gpar ^ 1u] = atomicAdd (&ctr->lc[par].work, (u32) FK_GROUP); }
      if (lane == 0) { T.ncand[(it + 2u) & 3u] = 0; T.ncand2 = 0; }      // (zeroed two tiles ahead; the second chance's: a barrier ahead)
    }
    u32 S32 = 0, L32 = 0, N32 = 0;
    const u32 pred_now = pred;
    u32 x[8];
    // ---- phase 1: 32 bytes per lane -> codes, run starts, letters ---------------------------------------------
    // (with_n: the tile's second chance, see below -- 'N' is let through and its positions are gathered as well)
    auto classify = [&] (auto with_n) -> u32 {
      constexpr bool NP = decltype (with_n)::value;
      // the word in front: the last word of the lane before (one DPP move); the wave's first lane has it from `pred`
      const u32 prevw = (u32) __builtin_amdgcn_update_dpp ((int) pred_now, (int) x[7], 0x138, 0xF, 0xF, false);   // wave_shr:1
      u32 selp = prevw & M07, bad = 0, r[8], sc[4] = {0, 0, 0, 0}, lc[4] = {0, 0, 0, 0}, nc[4] = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const u32 w = x[j];
        const u32 sel = w & M07;
        // every byte must be the table's entry for its low three bits: 1 'A', 2 '\n', 3 'C', 4 'T', 7 'G' (entries 0, 5, 6
        // hold bytes with other low bits: they can never match; the second chance has 'N' at 6)
        const u32 rec = __builtin_amdgcn_perm (NP ? 0x474E0054u : 0x47000054u, 0x430A4101u, sel);
        bad = __builtin_amdgcn_bitop3_b32 (bad, w, rec, BITOP3_OR_XOR);
        // 2-bit code (A 0, C 1, G 2, T 3; N 0; the delimiter 3, which no record ever packs) by table look-up on the low three
        // bits (one v_perm; round 2 took bits 1-2 of b ^ (b >> 1): a shift and a v_bitop3, and codes that sat one bit up),
        // gathered 4 bytes -> 8 bits
        const u32 cd = __builtin_amdgcn_perm (0x02000003u, 0x01030000u, sel);
        r[j] = __builtin_amdgcn_udot4 (cd, 0x40100401u, 0u, false);
        // letters have bit 6 ('\n' has not): 64 x the byte of 8 flags per pair of words
        const u32 wts = (j & 1) ? 0x80402010u : 0x08040201u;
        lc[j >> 1] = __builtin_amdgcn_udot4 (w & M40, wts, lc[j >> 1], false);
        // run start: low three bits differ from the byte before
        const u32 d = sel ^ __builtin_amdgcn_alignbit (sel, selp, 24);
        const u32 nz = __builtin_amdgcn_perm (0x01010101u, 0x01010100u, d);       // byte != 0 -> 1
        sc[j >> 1] = __builtin_amdgcn_udot4 (nz, wts, sc[j >> 1], false);
        if constexpr (NP) nc[j >> 1] = __builtin_amdgcn_udot4 (__builtin_amdgcn_perm (0x00010000u, 0u, sel), wts, nc[j >> 1], false);
        selp = sel;
      }
      // four gathered bytes -> one word with two byte permutes and an OR (as shifts and ORs the compiler spent seven
      // instructions per word here, 26 per tile and lane for the three planes; now 13)
      auto pack4 = [] (u32 b0, u32 b1, u32 b2, u32 b3) {
        return __builtin_amdgcn_perm (b1, b0, 0x0c0c0400u) | __builtin_amdgcn_perm (b3, b2, 0x04000c0cu);
      };
      const u32 code_lo = pack4 (r[0], r[1], r[2], r[3]);
      const u32 code_hi = pack4 (r[4], r[5], r[6], r[7]);
      S32 = pack4 (sc[0], sc[1], sc[2], sc[3]);
      {                                                   // (the letter flags come 64-fold: bit 6 of the bytes)
        const u32 u = lc[0] | (lc[1] << 8), v = lc[2] | (lc[3] << 8);
        L32 = (u >> 6) | (v << 10);
      }
      *reinterpret_cast<uint2 *> (&T.code[2 * tid]) = make_uint2 (code_lo, code_hi);
      T.st[tid] = S32;
      T.lt[tid] = L32;
      if constexpr (NP) { N32 = nc[0] | (nc[1] << 8) | (nc[2] << 16) | (nc[3] << 24); T.np[tid] = N32; }
      return bad;
    };
    // ---- phase 2: candidate tract starts among this lane's 32 positions ------------------------------------------
    // (the next lane's run starts come by DPP; the wave's last lane assumes none, i.e. that runs go on: phase 3 checks
    // the length anyway.)  count_addr: the LDS word that counts the tile's candidates.
    auto find_candidates = [&] (u32 count_addr, bool n_tile) {
      const u32 nx = (u32) __builtin_amdgcn_update_dpp (0, (int) S32, 0x130, 0xF, 0xF, false);   // wave_shl:1
      u32 cand = S32 & L32 & own;
      // no run start at the next mprime - 1 positions (the usual minimum lengths without a loop: its scalar bookkeeping
      // costs more than the vector work)
      {
        // (minimum lengths 2, 3, 4 through masks in VGPRs: a branch on mprime here cost a dozen scalar instructions per tile)
        const u32 a1 = __builtin_amdgcn_alignbit (nx, S32, 1u), a2 = __builtin_amdgcn_alignbit (nx, S32, 2u), a3 = __builtin_amdgcn_alignbit (nx, S32, 3u);
        const u32 t = __builtin_amdgcn_bitop3_b32 (a1, a2, vm3, 0xF8);      // a1 | (a2 & m3)
        cand = __builtin_amdgcn_bitop3_b32 (cand, t, a3 & vm4, 0x10);       // cand & ~t & ~(a3 & m4)
        int mp_now = mprime;
        asm volatile ("" : "+s"(mp_now));                 // (compared afresh: one s_cmp instead of a mask kept across the loop)
        if (mp_now > 4) for (int j = 4; j < mp_now; j++) cand &= ~__builtin_amdgcn_alignbit (nx, S32, (u32) j);
      }
      // (a run of 'N' long enough to count takes its context from the tract before it, reference src/hopo_counter.c:246-248:
      // the general kernel's business)
      if (n_tile && (cand & N32)) T.ncand2 = 0x40000000u;
      const u32 n = (u32) __popc (cand);
      // (tried: every lane reserves its own entries with one LDS atomic on the count word instead of the prefix sum -- 7 M
      // fewer vector instructions, but 64 adds on one address hold the LDS pipe for as many cycles: + 17 % time)
      const u32 incl = wave_inclusive_scan (n);
      const u32 total = (u32) __builtin_amdgcn_readlane ((int) incl, 63);
      u32 wraw;
      lds_add_issue (count_addr, total, wraw);
      const u32 p0 = (u32) (FK_UNIT * tid);
      const u32 wbase = lds_collect (wraw);
      // (a wave whose candidates would not all fit leaves its list alone: the tile is given up below)
      if (wbase + total <= (u32) FK_MAXCAND) {
        u32 at = wbase + incl - n;
        // (tried: a loop on "any lane has one left" as a scalar branch, with the idle lanes writing to spare entries -- no
        // exec mask to keep per iteration, 11 M fewer scalar instructions per launch, and 4 % slower)
        while (cand) {
          const u32 b = (u32) __ffs ((int) cand) - 1u;
          cand &= cand - 1u;
          T.cand[at] = (unsigned short) (p0 | b);
          at++;
        }
      }
    };
    {
      // This wave's part of the tile has landed in raw.  (Tried in round 3: a counted wait -- vmcnt(7) when a full partition
      // pass, whose last seven vector-memory operations are its stores, has run since the prefetch -- so that the stores
      // need not be waited for.  It needs the predecessor word loaded outside the compiler's view, into a register that
      // the compiler then copies before the word has arrived; through LDS it would cost what it gains, 1.7 %.)
      asm volatile ("s_waitcnt vmcnt(0)" ::: "memory");
      if constexpr (LOG) sink.collect ();
      const uint4 va = raw[2 * tid], vb = raw[2 * tid + 1];
      x[0] = va.x; x[1] = va.y; x[2] = va.z; x[3] = va.w; x[4] = vb.x; x[5] = vb.y; x[6] = vb.z; x[7] = vb.w;
      if (!((u32) (tile - 1) < (u32) t_hi)) {            // (uniform; the stream's first and last tiles) chunks that are not wholly inside the stream: byte by byte
        const long p0 = tile * (long) FK_OWN - FK_HL + 32l * tid;
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const long g = p0 + 16l * h;
          if (!(g >= 0 && g + 16 <= n_bytes)) {
            const EdgeChunk e = edge_chunk (seq, n_bytes, g);      // (outside the stream everything is a read delimiter)
            // (the wait for whatever the call left in flight, here: left to the compiler it sits where the two paths meet,
            // in the classification of EVERY tile, as vmcnt(0) -- which would also wait for the stores of a partition pass)
            __builtin_amdgcn_s_waitcnt (0x0F70);          // vmcnt(0) only
            x[4 * h] = e.x; x[4 * h + 1] = e.y; x[4 * h + 2] = e.z; x[4 * h + 3] = e.w;
          }
        }
      }
      if (classify (std::false_type ())) T.ncand[slot] = 0x40000000u;   // (more candidates than any tile has: looked at below; later atomic adds keep it so)
    }
    // the tile after this one
    int nt = tile + 1;
    if (nt >= grp_end) nt = __builtin_amdgcn_readfirstlane ((int) T.grp[gpar ^ 1u]);
    asm volatile ("s_waitcnt lgkmcnt(0)" ::: "memory");   // raw has been read: it may be refilled
    prefetch (nt);

    find_candidates (ncand_addr + 4u * slot, false);
    // the records staged so far, exactly: read BEFORE the barrier -- between the barrier that ended the tile before and
    // this one nobody appends, so every wave reads the same number; behind the barrier the quick waves are already
    // appending this tile's records while a slow one has yet to look (seen: one scan in fifty lost some eighty records
    // when a wave got a larger number, partitioned on its own schedule and its barriers paired up with the others' wrongly)
    const u32 staged_v = SL.n;
    if constexpr (LOG) sink.tile_top (staged_v);
    lds_barrier ();

    // ---- phase 3: one lane per candidate ----------------------------------------------------------------------
    const u32 ncand_all = (u32) __builtin_amdgcn_readfirstlane ((int) T.ncand[slot]);
    // (`bound` has counted candidates, of which one in eight is not recorded -- with the true count the buffer is
    // partitioned when it is full)
    sink.bound = LOG ? 0u : (u32) __builtin_amdgcn_readfirstlane ((int) staged_v);
    u32 ncand_now = ncand_all;
    if (ncand_all >= 0x40000000u) {
      // Second chance for a tile with a byte outside the five: if all such bytes are 'N' (the no-call of every sequencer),
      // classify again with 'N' let through (it packs as code 0 like 'A' -- what the reference's table gives it in a flank
      // read forwards), gather where the 'N's are, find the candidates again, and let phase 3 read the tracts that have
      // one within their 2k + length positions from the stream.  Anything else -- lower case, U, IUPAC codes, a countable
      // run of 'N' -- still sends the tile to the general kernel.  (The bytes are still in registers; the tile costs
      // two more barriers and a second classification, a fraction of what the general kernel takes for it.)
      const u32 bad2 = classify (std::true_type ());
      if (bad2) T.ncand2 = 0x40000000u;
      lds_barrier ();
      find_candidates ((u32) (size_t) (lptr_t) &T.ncand2, true);
      lds_barrier ();
      ncand_now = (u32) __builtin_amdgcn_readfirstlane ((int) T.ncand2);
    }
    const bool give_up = ncand_now > (u32) FK_MAXCAND;    // (too many candidates, or a byte that is not for this kernel)
    if (give_up) {
      // (listed in batches: one atomic with a return value per tile, on one address for the whole grid, cost 4.6 us each
      // when every tile of a stream was given up -- more than scanning the tile)
      if (tid == 0) T.sbuf[n_sbuf] = (u32) tile;
      if (++n_sbuf == 32u) flush_slow ();
    }
    else {
      const int ncand = (int) ncand_now;
      // room for all of the tile's candidates (four tiles out of five): one reservation, none per round
      const bool all_fit = sink.bound + (u32) ncand <= (u32) sink.S;
      if (all_fit) sink.bound += (u32) ncand;
      if constexpr (W != 1) {                           // k > 12: two windows per plane (the flanks do not fit one with the tract)
        const long g0 = tile * (long) FK_OWN - FK_HL;
        const bool n_tile = ncand_all >= 0x40000000u;
        for (int cb0 = 0; cb0 < ncand; cb0 += FK_BLOCK) {
          if (!all_fit) sink.reserve1 ((u32) min (ncand - cb0, FK_BLOCK));   // (may partition)
          if (cb0 + 64 * wave >= ncand) continue;          // (whole waves without a candidate in this round)
          const int ci = cb0 + tid;
          bool have = false;
          u64 c0 = 0, c1 = 0;
          u32 base = 0, len10 = 0, flag = 0;
          if constexpr (W == 2) {
            // Straight-line path (round 3) for a tract whose k + length + k positions fit one 64-bit window of the planes
            // -- everything else, rare, goes through fast_tract below -- as in the one-word kernel: lanes past the list's
            // end redo its last entry and are masked at the end; the run starts from s + 1, the letters and the codes from
            // s - k are read together (three words each), the right flank's codes behind them once the run's end is known.
            const bool valid = ci < ncand;
            const u32 s = T.cand[min (ci, ncand - 1)];
            const u32 q = s + 1u, u = s - (u32) k;
            const u32 *ps = &T.st[q >> 5], *pl = &T.lt[u >> 5], *pc = &T.code[u >> 4];
            u32 s0 = ps[0], s1 = ps[1], s2 = ps[2], l0 = pl[0], l1 = pl[1], l2 = pl[2], w0 = pc[0], w1 = pc[1], w2 = pc[2];
            asm volatile ("" : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(l0), "+v"(l1), "+v"(l2), "+v"(w0), "+v"(w1), "+v"(w2));
            const u64 ns = ((u64) __builtin_amdgcn_alignbit (s2, s1, q) << 32) | __builtin_amdgcn_alignbit (s1, s0, q);
            const u32 len = (u32) __builtin_ctzll (ns | (1ull << 63)) + 1u;     // (no run start in 64 positions: 64, which does not fit)
            const int room = 64 - (int) (len + 2u * (u32) k);
            const bool fits = room >= 0;
            const u32 rpos = s + (fits ? len : 0u);          // (first position behind the tract; kept inside the planes otherwise)
            const u32 *pr = &T.code[rpos >> 4];
            const u32 r0 = pr[0], r1 = pr[1], r2 = pr[2];
            const u64 notl = ~(((u64) __builtin_amdgcn_alignbit (l2, l1, u) << 32) | __builtin_amdgcn_alignbit (l1, l0, u));
            const u64 km = kmask (k);
            const u64 L64 = ((u64) __builtin_amdgcn_alignbit (w2, w1, 2u * u) << 32) | __builtin_amdgcn_alignbit (w1, w0, 2u * u);
            const u64 R64 = ((u64) __builtin_amdgcn_alignbit (r2, r1, 2u * rpos) << 32) | __builtin_amdgcn_alignbit (r1, r0, 2u * rpos);
            const u64 left = L64 & km, right = R64 & km;
            const u32 cb = (u32) (L64 >> (2 * k)) & 3u;      // the tract's base (2k <= 56: inside the window)
            u64 nl2 = 0, nr2 = 0;
            if (n_tile) {                                   // (uniform) 'N's in the flanks: forward code 3 where the strand is turned (see fast_tract)
              const u32 kb32 = (1u << k) - 1u;
              const u32 nl = bits32 (T.np, (int) u) & kb32, nr = bits32 (T.np, (int) rpos) & kb32;
              if (nl | nr) { nl2 = spread_pairs (nl); nr2 = spread_pairs (nr); }
            }
            const bool rev = cb >= 2u;
            const u64 rc0 = revcomp_k (right | nr2, k), rc1 = revcomp_k (left | nl2, k);
            c0 = rev ? rc0 : left; c1 = rev ? rc1 : right;
            base = rev ? 3u - cb : cb; flag = rev ? 2u : 1u; len10 = len;
            have = valid && fits && (notl << (room & 63)) == 0ull && (int) len >= mprime;
            if (valid && !fits) have = fast_tract<false> (T, seq, n_bytes, g0, (int) s, k, mprime, c0, c1, base, len10, flag, n_tile);
          }
          else if (ci < ncand) have = fast_tract<false> (T, seq, n_bytes, g0, (int) T.cand[ci], k, mprime, c0, c1, base, len10, flag, n_tile);
          const u64 okm = __builtin_amdgcn_ballot_w64 (have);
          u32 araw;
          lds_add_issue (sink.count_addr (), (u32) __builtin_popcountll (okm), araw);
          const u32 at = lds_collect (araw) + (u32) __builtin_amdgcn_mbcnt_hi ((u32) (okm >> 32), __builtin_amdgcn_mbcnt_lo ((u32) okm, 0u));
          if (have) sink.store_fields (at, c0, c1, base, len10, flag);
        }
      }
      else
      for (int cb0 = 0; cb0 < ncand; cb0 += FK_BLOCK) {
        // Straight-line path for a tract whose k + length + k positions fit one 32-bit window (everything else is
        // `general`), without branches: lanes past the list's end work on its last entry again and are masked out at the
        // end.  The windows depend on s alone, so all their LDS reads are in flight together: run starts from s + 1,
        // letters from s - k, and 64 bits of codes from s - k (left flank, tract, right flank).
        if (!all_fit) sink.reserve1 ((u32) min (ncand - cb0, FK_BLOCK));    // (may partition: before anything of this round is in registers)
        if (cb0 + 64 * wave >= ncand) continue;            // (whole waves without a candidate in this round)
        const int ci = cb0 + tid;
        const bool valid = ci < ncand;
        const u32 s = T.cand[min (ci, ncand - 1)];
        const u32 q = s + 1u, u = s - vk;
        // (tried: the word addresses as shift + v_lshl_add_u32 on the planes' LDS addresses, two instructions per plane
        // instead of the compiler's three -- the three base addresses in VGPRs were three registers too many at this
        // kernel's 128-register edge once the counted wait below needed one)
        const u32 *ps = &T.st[q >> 5], *pl = &T.lt[u >> 5], *pc = &T.code[u >> 4];
        u32 s0 = ps[0], s1 = ps[1], l0 = pl[0], l1 = pl[1], w0 = pc[0], w1 = pc[1], w2 = pc[2];
        // (pinned: left alone the compiler waits for the run starts before it asks for the codes, and reads the letters
        // only inside a branch it makes up -- three LDS round trips in a row instead of one)
        asm volatile ("" : "+v"(s0), "+v"(s1), "+v"(l0), "+v"(l1), "+v"(w0), "+v"(w1), "+v"(w2));
        // run end: first run start after s (bit 31 set: "none in 32 positions" reads as a run of 32, which is general)
        const u32 len = (u32) __builtin_ctz (__builtin_amdgcn_alignbit (s1, s0, q) | 0x80000000u) + 1u;
        const u32 need = len + vk2;                        // k letters, the tract, k letters
        const u32 room = v32 - need;                       // (negative: the window is too short -> `general`)
        const u32 notl = ~__builtin_amdgcn_alignbit (l1, l0, u);
        // recorded: fits the window, letters all the way, long enough -- as one integer so that it costs vector
        // instructions only (the compiler turns `a && b && c` into an exec region of six scalar instructions)
        // (lanes past the list's end: a minimum length that nothing reaches)
        const u32 bad = __builtin_amdgcn_bitop3_b32 (notl << (room & 31u), room >> 31, (len - (valid ? vmp : 0x1000u)) >> 31, 0xFE);
        const bool ok = bad == 0u;
        if (valid && (int) room < 0) {                     // (rare) the long tracts: appended on their own (before this wave's atomic is issued: its result register must not live across a call)
          const u64 rec = fast_general_tract (T, seq, n_bytes, tile * (long) FK_OWN - FK_HL, (int) s, k, mprime, (ncand_all >= 0x40000000u));
          if (rec != 0ull) sink.store1 (atomicAdd (&sink.L.n, 1u), (u32) rec, (u32) (rec >> 32));
        }
        // whether the tract is recorded is known: its slot in the staging buffer is asked for now (an LDS atomic per
        // wave) and the record is worked out while that is on its way
        const u64 okm = __builtin_amdgcn_ballot_w64 (ok);
        u32 araw;
        lds_add_issue (sink.count_addr (), (u32) __builtin_popcountll (okm), araw);
        const u32 sh = u + u;
        const u32 clo = __builtin_amdgcn_alignbit (w1, w0, sh), chi = __builtin_amdgcn_alignbit (w2, w1, sh);
        const u32 l = clo & vkm;
        const u32 cb = (clo >> vk2) & 3u;                  // the tract's base
        const u32 r = (u32) ((((u64) chi << 32) | clo) >> (vk2 + len + len)) & vkm;
        // canonical orientation (reference: src/hopo_counter.c:233-246): T / G tracts store the reverse complement
        u32 rcl = revcomp_v32 (l, M55, vrs), rcr = revcomp_v32 (r, M55, vrs);
        if ((ncand_all >= 0x40000000u)) {                                       // (uniform) 'N's in the flanks: forward code 3 where the strand is turned (see fast_tract)
          const u32 nb = bits32 (T.np, (int) u);
          if ((nb << ((v32 - need) & 31u)) != 0u && need <= 32u) {
            rcl = revcomp_v32 (l | (u32) spread_pairs (nb & ((1u << k) - 1u)), M55, vrs);
            rcr = revcomp_v32 (r | (u32) spread_pairs ((nb >> ((u32) k + len)) & ((1u << k) - 1u)), M55, vrs);
          }
        }
        const bool rev = cb >= 2u;
        const u32 c0 = rev ? rcr : l, c1 = rev ? rcl : r;
        // base << 2 | flag << 3 by table look-up on cb: A (0, fwd) 8, C (1, fwd) 12, G (-> C, rev) 20, T (-> A, rev) 16
        // (looked up straight into the record's top byte: selector byte 3 = cb, the others "zero")
        const u32 fld24 = __builtin_amdgcn_perm (0u, 0x10140C08u, (cb << 24) | 0x000C0C0Cu);
        const u32 lo = c1 | (len << 24);
        const u32 hi = c0 | fld24;
        const u32 at = lds_collect (araw) + (u32) __builtin_amdgcn_mbcnt_hi ((u32) (okm >> 32), __builtin_amdgcn_mbcnt_lo ((u32) okm, 0u));
        if constexpr (LOG) sink.store1ok (ok, at, lo, hi, (u32) lane);
        else sink.store1v (ok ? at : (u32) sink.S + (u32) lane, lo, hi, vh0, vh1, vm27);   // (no record: a spare slot takes the write)
      }
    }
    lds_barrier ();
    if (nt >= grp_end) { gpar ^= 1u; grp_end = nt + FK_GROUP; }
    tile = nt;
    it++;
  }
  flush_slow ();
  sink.finish ();
}

// The record log of scan_fast_kernel<W, true> -> the hash buckets.  A workgroup takes log blocks in turn (static stride)
// and sorts one block per pass by bucket, a counting sort like StageSink's with the records held in registers from HBM
// to their sorted slot -- the same reservation protocol on the same bucket cursors and chunk table as every other
// producer of raw records.
#define PL_BLOCK 512
#define PL_WG_PER_CU 2
template <int W>
__global__ __launch_bounds__ (PL_BLOCK, PL_BLOCK * PL_WG_PER_CU / 256)
void partition_log_kernel (LogSpace LG, Buckets BK, DevCounters *ctr, int k)
{
  // One log block (TJ_LOGB words: 8192 one-word or 4096 two-word records, 16 words per thread) per pass, the records in
  // registers from the load to their place in the sorted buffer: count per bucket (LDS atomics) -- prefix, one
  // reservation per bucket, where the runs go (the owners, as in StageSink::partition_pass) -- every record straight to
  // its sorted slot in LDS (its rank: an LDS atomic on the bucket's running position) -- the sorted buffer out in runs,
  // coalesced.  Four barriers per block; two workgroups per CU cover each other's waits.  What bounds it is the memory
  // system: for the 10 M-read sample's one-word records 0.48 GB read in a line, 0.48 GB written in runs of 32 records to
  // 256 places (tools/ubench/write_runs.hip: that write pattern alone takes 0.16 ms); loading the next block's records
  // while this one is sorted and written changed nothing (tried, with 32 more registers).
  static_assert (W == 1 || W == 2, "the log holds one-word and two-word records");
  typedef StageLds<W, 2> Lds;
  __shared__ Lds L;
  constexpr u32 RB = TJ_LOGB / W;                        // records per block
  static_assert (Lds::S == (int) RB && Lds::WS == W, "one pass per log block");
  constexpr u32 RR = RB / PL_BLOCK;                      // records per thread
  static_assert (RR % 4 == 0, "bins are kept four to a register");
  const u32 tid = threadIdx.x, lane = tid & 63u;
  const u32 wave = (u32) __builtin_amdgcn_readfirstlane ((int) (tid >> 6));
  if (tid < TJ_P) L.hist[tid] = 0;
  u32 cur_j = TJ_EMPTY, cur_chunk = TJ_NOCHUNK;         // owner thread (tid < TJ_P): the chunk its bucket was written to last
  lds_barrier ();
  const u32 n_blocks = min (*LG.next, LG.n_blocks);
  // (blocks in turn, static: a shared work counter would be one more address that every workgroup of the grid adds to)
  u32 b = blockIdx.x;
  if (b >= n_blocks) return;
  u64 w[RR][W];
  u32 n = min (LG.count[b], RB), nn = 0;
  // a block's records, the part of it that was written: whole waves skip what lies behind the block's count (every scanning
  // workgroup leaves one block partly filled and one empty: a tenth of all blocks on the 10 M-read sample, nearly all of
  // them on a sparse one)
  auto load_block = [&] (u32 blk, u32 cnt) {
    const u64 *__restrict__ src = LG.log + ((u64) blk << TJ_LOGB_SHIFT);
    const u32 w0 = tid & ~63u;                            // (the wave's first thread: uniform)
#pragma unroll
    for (u32 r = 0; r < RR; r++) {
#pragma unroll
      for (int j = 0; j < W; j++) w[r][j] = 0;
      if (w0 + r * PL_BLOCK < cnt) {
        if constexpr (W == 1) w[r][0] = (src + r * PL_BLOCK)[tid];
        else { const ulonglong2 v = reinterpret_cast<const ulonglong2 *> (src + 2u * r * PL_BLOCK)[tid]; w[r][0] = v.x; w[r][1] = v.y; }
      }
    }
  };
  auto bucket_of = [&] (const u64 *rec) -> u32 {
    if constexpr (W == 1) return bucket_of_rec1 ((u32) rec[0], (u32) (rec[0] >> 32));
    else { u64 c0, c1; u32 base, len10, flag; unpack_raw<W> (rec, k, c0, c1, base, len10, flag); return bucket_of_key (c0, c1, base, len10); }
  };
  load_block (b, n);
  while (true) {
    const u32 bn = b + gridDim.x;
    const bool more = bn < n_blocks;                      // (uniform)
    if (more) nn = min (LG.count[bn], RB);                // (asked for now, looked at when this block is done)
    u32 tq = tid;
    asm volatile ("" : "+v"(tq));                         // (opaque: what the compiler can derive from tid alone it hoists out of the loop -- sixteen 64-bit offsets 8 i took 32 registers and went to scratch)
    u32 pk[RR / 4];
#pragma unroll
    for (u32 r = 0; r < RR / 4; r++) pk[r] = 0;
    if (n) {
      // ---- records per bucket
#pragma unroll
      for (u32 r = 0; r < RR; r++) {
        const u32 bin = bucket_of (w[r]);
        pk[r >> 2] |= bin << (8u * (r & 3u));
        if (tid + r * PL_BLOCK < n) atomicAdd (&L.hist[bin], 1u);
      }
      lds_barrier ();
      // ---- owners: prefix, reservation, where the run lives
      if (wave < TJ_P / 64) {
        const uint4 h4 = *reinterpret_cast<const uint4 *> (&L.hist[4 * lane]);
        const u32 tot = h4.x + h4.y + h4.z + h4.w;
        const u32 e0 = wave_inclusive_scan (tot) - tot;
        if ((lane >> 4) == wave) *reinterpret_cast<uint4 *> (&L.offs[4 * lane]) = make_uint4 (e0, e0 + h4.x, e0 + h4.x + h4.y, e0 + h4.x + h4.y + h4.z);
        const u32 cnt = L.hist[tid], off = L.offs[tid];
        u64 a1 = 0, a2 = 0;
        u32 thr = off + cnt;
        if (cnt) {
          const u32 p0 = atomicAdd (&BK.cursors[tid * TJ_CSTRIDE], cnt);
          const u32 ch = (u32) TJ_CH0 << BK.ch_shift;
          bucket_claim_ahead_range (BK, tid, p0, cnt, ctr);   // (a run of up to a block's records may hold more than one chunk's first record)
          const u32 j0 = chunk_of_pos (BK, p0), j1 = chunk_of_pos (BK, p0 + cnt - 1);
          if (j0 != cur_j) { cur_j = j0; cur_chunk = bucket_chunk_id (BK, tid, j0, true, ctr); }
          if (cur_chunk != TJ_NOCHUNK) a1 = (u64) (size_t) (BK.pool + ((u64) cur_chunk * ch + (p0 - j0 * ch)) * W) - (8ull * W) * off;
          if (j1 != j0) {                                 // the run crosses into the next chunk (chunks are longer than a log block: at most once)
            thr = off + ((j0 + 1u) * ch - p0);
            cur_j = j0 + 1u; cur_chunk = bucket_chunk_id (BK, tid, j0 + 1u, true, ctr);
            if (cur_chunk != TJ_NOCHUNK) a2 = (u64) (size_t) (BK.pool + ((u64) cur_chunk * ch) * W) - (8ull * W) * thr;
          }
        }
        reinterpret_cast<uint4 *> (L.gbase)[tid] = make_uint4 ((u32) a1, (u32) (a1 >> 32) | (thr << 16), (u32) a2, (u32) (a2 >> 32));
      }
      lds_barrier ();
      if (tid < TJ_P) L.hist[tid] = 0;                    // (for the next block; the ranks below count in offs)
      // ---- every record to its sorted slot (offs[bucket] runs from the bucket's first slot to its last)
#pragma unroll
      for (u32 r = 0; r < RR; r++)
        if (tid + r * PL_BLOCK < n) {
          const u32 bin = (pk[r >> 2] >> (8u * (r & 3u))) & 255u;
          const u32 d = atomicAdd (&L.offs[bin], 1u);
#pragma unroll
          for (int j = 0; j < W; j++) L.rec[d * W + j] = w[r][j];
          L.bin[d] = (unsigned char) bin;
        }
      lds_barrier ();
      // ---- copy-out: sorted slot i -> its place in the bucket's run
      for (u32 r0 = 0; r0 < RR; r0 += 4) {
        if (r0 * PL_BLOCK >= n) break;
        u32 cb[4]; uint4 e[4]; u64 cw[4][W];
#pragma unroll
        for (u32 h = 0; h < 4; h++) cb[h] = L.bin[tq + (r0 + h) * PL_BLOCK];
#pragma unroll
        for (u32 h = 0; h < 4; h++) {
          e[h] = reinterpret_cast<const uint4 *> (L.gbase)[cb[h]];
#pragma unroll
          for (int j = 0; j < W; j++) cw[h][j] = L.rec[(tq + (r0 + h) * PL_BLOCK) * W + j];
        }
#pragma unroll
        for (u32 h = 0; h < 4; h++) {
          const u32 i = tq + (r0 + h) * PL_BLOCK;
          const u64 a = (i < (e[h].y >> 16)) ? (((u64) (e[h].y & 0xFFFFu) << 32) | e[h].x) : (((u64) e[h].w << 32) | e[h].z);
          if (i < n && a != 0ull) {
            typedef __attribute__((address_space(1))) u64 *gwords_t;
            gwords_t q = (gwords_t) (a + (u64) (8u * W * i));
#pragma unroll
            for (int j = 0; j < W; j++) q[j] = cw[h][j];
          }
        }
      }
      lds_barrier ();                                     // the sorted buffer is free again
    }
    if (!more) break;
    load_block (bn, nn);
    n = nn; b = bn;
  }
}

template <int W>
__global__ void nrun_fixup_bins_kernel (const uint8_t *__restrict__ seq, long n_bytes, int k, int mprime,
                                        Buckets BK, DevCounters *ctr, const FixEntry *fix, u32 fix_cap, int par)
{
  nrun_fixup_entries<W> (seq, n_bytes, k, mprime, BK, ctr, fix, fix_cap, par, blockIdx.x * (u64) blockDim.x + threadIdx.x, (u64) gridDim.x * blockDim.x);
}

// host hopo_element array (40 B each) -> buckets
template <int W>
__global__ void bin_elems_kernel (const u64 *__restrict__ elems5, long n, int k, Buckets BK, DevCounters *ctr)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    const u64 m = elems5[5 * i + 2];
    bucket_insert_slow<W> (elems5[5 * i], elems5[5 * i + 1], (u32) (m & 3ull), (u32) ((m >> TJ_META_LEN_SHIFT) & 0x3FFull),
                           (u32) ((m >> TJ_META_FLAG_SHIFT) & 3ull), k, BK, ctr);
  }
}

// buckets -> flat list of 24-byte raw records, padding skipped (test aid; order is irrelevant)
template <int W>
__global__ void unpack_buckets_kernel (Buckets BK, int k, u64 *__restrict__ out, u64 cap, u64 *n_out)
{
  const u32 b = blockIdx.x;
  const u32 n = BK.cursors[b * TJ_CSTRIDE];
  for (u32 i = threadIdx.x; i < n; i += blockDim.x) {
    u64 c0, c1; u32 base, len10, flag;
    const u64 at = bucket_slot (BK, b, i, false, nullptr);
    if (at == ~0ull) continue;
    unpack_raw<W> (BK.pool + at * W, k, c0, c1, base, len10, flag);
    if (flag == 3u) continue;
    const u64 o = atomicAdd (n_out, 1ull);
    if (o < cap) { u64 *q = out + 3 * o; q[0] = c0; q[1] = c1; q[2] = make_meta (base, len10, flag); }
  }
}

// chunk 0 of every bucket
__global__ void init_table_kernel (u32 *table, u32 maxj, u32 *pool_next)
{
  const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < TJ_P) table[(u64) b * maxj] = b;
  if (b == 0) *pool_next = TJ_P;
}

// empty buckets: cursors 0, every bucket owns chunk b as its chunk 0, the rest of the table unclaimed, pool_next = TJ_P.
// One workgroup per bucket; only the row entries the bucket can have claimed are rewritten (its records / chunk + the
// one claimed ahead), unless the whole row is asked for.
__global__ void clear_buckets_kernel (u32 *cursors, DevCounters *ctr, u32 *table, u32 maxj, int ch_shift, FinCounts *fin, u32 *bins, int nbins,
                                      DevCounters *snap_ctr, u32 *snap_cursors, FinPlan *plan, u32 *__restrict__ fine = nullptr, int fine_bits = 0)
{
  const u32 b = blockIdx.x;
  if (snap_ctr) {                                       // (every workgroup reads its own cursor, workgroup 0 the rest: before anything is zeroed)
    if (threadIdx.x == 0) {
      snap_cursors[b] = cursors[b * TJ_CSTRIDE];
      if (b == 0) {
        snap_cursors[TJ_P] = cursors[TJ_P * TJ_CSTRIDE];
        // The kept count and the overflow flag as a kernel boundary shows them.  plan_tail read them inside the
        // aggregation, from its last workgroup, through relaxed atomics and no fence (a fence there doubled the kernel's
        // time): the host compares the two readings and runs the ordering step again if they ever differ.
        if (plan) { plan->n1_exact = (long) fin->n_kept; plan->ovf_exact = fin->overflow; }
      }
    }
    if (b == 0) for (u32 i = threadIdx.x; i < sizeof (DevCounters) / 4; i += blockDim.x) reinterpret_cast<u32 *> (snap_ctr)[i] = reinterpret_cast<const u32 *> (ctr)[i];
    __syncthreads ();
  }
  // the scan counters as well (all but n_undefined, which counts from reset to reset): a reset right after a finalise
  // then needs no memset of its own
  if (b == 0) for (u32 i = threadIdx.x; i < sizeof (DevCounters) / 4; i += blockDim.x) if (i != offsetof (DevCounters, n_undefined) / 4 && i != offsetof (DevCounters, n_undefined) / 4 + 1) reinterpret_cast<u32 *> (ctr)[i] = 0;
  if (table) {
    u32 used = maxj;
    if (ch_shift >= 0) used = min (maxj, ((cursors[b * TJ_CSTRIDE] / TJ_CH0) >> ch_shift) + 3u);
    for (u32 j = threadIdx.x; j < used; j += blockDim.x) table[(u64) b * maxj + j] = j ? TJ_EMPTY : b;
  }
  if (fine) {
    // The aggregation before this kernel has counted the records it kept into 2^fine_bits bins (the finest partition the
    // ordering step can ask for); its plan says how many leading bits the step uses: a bin of the step is a run of
    // 2^shift fine ones (a bin is a prefix of the key).  Summed here, one run per thread, which also zeroes what it has
    // read for the next aggregation (loads first: a store to the array between two loads of it serialises them) -- this
    // replaces the step's counting pass over the kept records.  No usable plan: the counts go, the step counts again.
    const int gid = (int) (b * blockDim.x + threadIdx.x), gsz = (int) (gridDim.x * blockDim.x);
    if (plan->ok) {
      const int shift = fine_bits - plan->nbits, run = 1 << shift, nb = plan->nbins;
      for (int i = gid; i < nb; i += gsz) {
        u32 sum = 0;
        if (shift >= 2) {
          uint4 *f4 = reinterpret_cast<uint4 *> (fine) + (size_t) i * (run >> 2);
          for (int j = 0; j < (run >> 2); j++) { const uint4 v = f4[j]; sum += v.x + v.y + v.z + v.w; }
          for (int j = 0; j < (run >> 2); j++) f4[j] = make_uint4 (0, 0, 0, 0);
        }
        else {
          for (int j = 0; j < run; j++) sum += fine[(i << shift) + j];
          for (int j = 0; j < run; j++) fine[(i << shift) + j] = 0;
        }
        bins[i] = sum;
      }
    }
    else for (int i = gid; i < (1 << fine_bits); i += gsz) fine[i] = 0;
  }
  else if (bins) for (int i = (int) (b * blockDim.x + threadIdx.x); i < nbins; i += (int) (gridDim.x * blockDim.x)) bins[i] = 0;
  __syncthreads ();
  if (threadIdx.x == 0) { cursors[b * TJ_CSTRIDE] = 0; if (b == 0) { cursors[TJ_P * TJ_CSTRIDE] = TJ_P; fin->n_kept = 0; fin->overflow = 0; fin->pad = 0; } }
}

// chunk table with a longer row
__global__ void table_relayout_kernel (const u32 *__restrict__ old, u32 old_maxj, u32 *__restrict__ neu, u32 new_maxj)
{
  const u32 b = blockIdx.x;
  for (u32 j = threadIdx.x; j < old_maxj; j += blockDim.x) neu[(u64) b * new_maxj + j] = old[(u64) b * old_maxj + j];
}

// ---------------------------------------------------------------------------------------------------------------
// aggregation: one workgroup per bucket streams its raw records through an LDS hash table keyed by
// (base, context, stored length), counting the two strands separately (reference: the qsort + run-length pass of
// src/hopo_counter.c:351-365), then applies the strand / singleton filter (:367-374) and appends the survivors, as
// 24-byte records carrying count and canon_flag, to the kept list.  A table that fills up closes (no new keys; records
// of absent keys go to a second pool) and the leftovers are aggregated in further rounds; a key is always entirely in
// one round, so rounds never split a count.  One kernel per record width; aggregate1_kernel carries the commentary.

#define AG_BLOCK    1024
#define AG_NCH      512                 // chunk ids of a bucket cached in LDS (longer buckets look the rest up in the table)

// ---- W = 1 (k <= 12): the whole reduction key is the record word without its strand flag, so one 64-bit LDS
// compare-and-swap per probe decides "new key / same key / other key" -- no tag, no publish step, no key read-back.
#define AG1_S        8192
#define AG1_CLOSE_AT 4864                // typical overshoot: a few keys; worst case one per lane (1024): 72 % full
#define AG1_R        4                   // records in flight per lane
#define AG1_MARK     (~0ull)             // a key has bits 59-63 clear

#define BS_MAXBITS   16                  // (bins of the ordering step: see bin_count_kernel)
__host__ __device__ static inline int cov_table_bits (long n1) { int b = 10; while ((1l << b) < 4 * n1 && b < 31) b++; return b; }   // 2 n1 entries at most: half full
// The coverage table's keys are flanks cut to 31 bits (src/hopo_counter.c:419-438): with 2k <= 31 there are 4^k of them, and
// when that is no more than the hash table would have slots the table is addressed by the key itself -- a quarter of the
// memory to zero and to look through at k = 10, and a plain add instead of a compare-and-swap round trip per record.
__host__ __device__ static inline int cov_plan_bits (long n1, int k, int *direct)
{
  const int hb = cov_table_bits (n1), kb = 2 * k < 31 ? 2 * k : 31;
  *direct = kb <= hb ? 1 : 0;
  return kb <= hb ? kb : hb;
}
// bins of the finest partition the ordering step can ask for: the aggregation counts its kept records into them as it
// writes them (the sample's kept count, which decides how many leading bits the step really uses, is not known yet)
__host__ __device__ static inline int fine_bin_bits (int k) { return BS_MAXBITS < 1 + 4 * k ? BS_MAXBITS : 1 + 4 * k; }
__device__ __forceinline__ u32 bin_of_record (u64 c0, u64 c1, u64 meta, int k, int nbits);
__host__ __device__ static inline int bin_bits_for (long n1, int k)
{
  int nbits = 6;
  while (nbits < BS_MAXBITS && nbits < 1 + 4 * k && (48l << nbits) < n1) nbits++;    // ~24..48 records per bin: most of a wavefront's lanes busy
  return nbits < 1 + 4 * k ? nbits : 1 + 4 * k;
}
// The last workgroup of an aggregation to finish derives the sizes the ordering kernels work with (FinPlan) from the
// number of kept records: what a one-thread kernel launched behind the aggregation used to do, for 5 us of stream time.
// fin->pad counts the workgroups that are through (zero before every aggregation: here, and clear_buckets_kernel).
// the kept list is full: said with an atomic whose return the thread waits for (see plan_tail)
__device__ __forceinline__ void flag_kept_overflow (FinCounts *fin)
{
  u32 old = atomicOr (&fin->overflow, 1u);
  asm volatile ("" :: "v"(old));
}

__device__ __forceinline__ void plan_tail (FinCounts *fin, int k, long cap, FinPlan *plan)
{
  if (!plan) return;
  // (no __threadfence: at device scope it writes the XCD's L2 back, which doubled the aggregation's run time.  What the
  // last workgroup needs from the others went through atomics that their threads waited for -- the kept count, the
  // overflow flag -- before the barrier in front of their tick.)
  __syncthreads ();
  if (threadIdx.x == 0) {
    const u32 done = atomicAdd (&fin->pad, 1u);
    if (done == gridDim.x - 1u) {
      const long n1 = (long) __hip_atomic_load (&fin->n_kept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const u32 ovf = __hip_atomic_load (&fin->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      plan->n1 = n1; plan->kept_overflow = ovf;
      plan->nbits = bin_bits_for (n1, k); plan->nbins = 1 << plan->nbits;
      int direct;
      plan->log2t = cov_plan_bits (n1, k, &direct); plan->t = 1l << plan->log2t; plan->cov_direct = (u32) direct;
      plan->ok = (n1 > 0 && n1 <= cap && !ovf) ? 1 : 0;
      fin->pad = 0;
    }
  }
}

// The t-th batch a workgroup hands to its waves: the bucket is read FROM ITS END.  The order of the records does not matter to
// a hash aggregation, and what a bucket received last is what the 256 MB memory-side cache may still hold when the
// aggregation starts right behind the kernel that filled it: behind partition_log_kernel the waves' wait for their loads
// fell by more than half and the kernel from 0.160 to 0.137 ms (the time it takes behind the fused scan kernel).
// Returns a position >= n when the bucket is used up.
__device__ __forceinline__ u32 batch_start (u32 t, u32 n, u32 batch)
{
  const u32 nb = (n + batch - 1u) / batch;
  return t < nb ? (nb - 1u - t) * batch : n;
}

struct Agg1Lds
{
  u64 key[AG1_S];                       // record without its strand flag (never 0: the base next to an A tract is not A)
  u32 cnt[2 * AG1_S];                   // per slot: records seen on the forward / on the reverse strand
  u32 chunk[AG_NCH];                    // the bucket's chunk ids
  u32 n_claimed, n_ovf, total;
  u32 next_batch;                       // batches of 64 * AG1_R records are handed to the waves as they come for one
  u32 wsum[AG_BLOCK / 64];
};

__global__ __launch_bounds__ (AG_BLOCK)
void aggregate1_kernel (Buckets BK, u64 *ovf, int k, int remove_biased, u64 *__restrict__ kept, u64 kept_cap, FinCounts *fin,
                        long plan_cap, FinPlan *plan, u32 *__restrict__ fine, int fine_bits)
{
  __shared__ Agg1Lds L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32 bkt = blockIdx.x;
  u32 n = BK.cursors[bkt * TJ_CSTRIDE];
  if (n) for (u32 j = (u32) tid; j <= chunk_of_pos (BK, n - 1u) && j < AG_NCH; j += AG_BLOCK) L.chunk[j] = bucket_chunk_id (BK, bkt, j, false, nullptr);
  auto chunk_id = [&] (u32 j) { return j < AG_NCH ? L.chunk[j] : bucket_chunk_id (BK, bkt, j, false, nullptr); };

  // records that do not fit a round's table go to the same place in a second pool (`ovf`) and are read from there in
  // the next round, whose own leftovers go back to the first pool: no wave ever writes where another may still read,
  // so the waves of a round run free of each other (no barrier in the record loop).
  const u64 *src = BK.pool;
  u64 *dst = ovf;
  while (n > 0) {
    for (int i = tid; i < AG1_S; i += AG_BLOCK) { L.key[i] = 0; L.cnt[2 * i] = 0; L.cnt[2 * i + 1] = 0; }
    if (tid == 0) { L.n_claimed = 0; L.n_ovf = 0; L.next_batch = 0; }
    __syncthreads ();

    // AG1_R records per lane are in flight while the previous AG1_R are inserted: with one 8-byte load per lane the
    // kernel sat at latency x (8 KB per CU in flight) = 1.4 TB/s whatever the table did.
    u64 wn[AG1_R];
    u32 vn = 0;
    // A batch is 64 * AG1_R consecutive records of the bucket: less than a chunk, so it lies in at most two chunks and
    // everything about them is wave-uniform (chunk ids come from LDS: no global look-up whose wait would also wait
    // for the records in flight).
    auto fetch = [&] (u32 b0) {
      vn = 0;
#pragma unroll
      for (int r = 0; r < AG1_R; r++) wn[r] = 0;
      if (b0 >= n) return;
      const u32 ch = (u32) TJ_CH0 << BK.ch_shift;
      const u32 j0 = chunk_of_pos (BK, b0), bound = (j0 + 1u) * ch;
      if (b0 + 64u * AG1_R <= min (n, bound) && j0 < AG_NCH) {      // a whole batch inside one chunk (nearly all of them):
        const u32 c0s = (u32) __builtin_amdgcn_readfirstlane ((int) L.chunk[j0]);   // scalar address arithmetic, four plain loads
        if (c0s != TJ_NOCHUNK) {
          const u64 *q = src + ((u64) c0s * ch + (b0 - j0 * ch)) + (u32) lane;
#pragma unroll
          for (int r = 0; r < AG1_R; r++) wn[r] = q[64 * r];
          vn = (1u << AG1_R) - 1u;
          return;
        }
      }
      const u32 c0 = chunk_id (j0), c1 = (bound < n) ? chunk_id (j0 + 1u) : TJ_NOCHUNK;
      const u64 off0 = (u64) c0 * ch - (u64) j0 * ch, off1 = (u64) c1 * ch - (u64) bound;   // record index -> pool index
#pragma unroll
      for (int r = 0; r < AG1_R; r++) {
        const u32 idx = b0 + (u32) r * 64u + (u32) lane;
        const bool hi = idx >= bound;
        if (idx < n && (hi ? c1 : c0) != TJ_NOCHUNK) { vn |= 1u << r; wn[r] = src[(hi ? off1 : off0) + idx]; }
      }
    };
    // Waves take batches of 64 * AG1_R consecutive records as they become free (one LDS atomic per batch): with a fixed
    // share per wave the slower waves of a SIMD finished a third of the round after the faster ones had started to wait.
    auto next_batch = [&] () {
      u32 b = 0;
      if (lane == 0) b = atomicAdd (&L.next_batch, 1u);
      return batch_start ((u32) __builtin_amdgcn_readfirstlane ((int) b), n, 64u * AG1_R);
    };
    u32 b_next = next_batch ();
    fetch (b_next);
    while (b_next < n) {
      const u32 b0 = b_next;
      (void) b0;
      // this round's records have arrived (fetched one round ago).  The registers pass through the asm so that the
      // compiler stops tracking them as pending loads: otherwise it waits for them again at their first use -- after
      // the next round's loads have been issued, i.e. for those as well (vmcnt counts in order).
      asm volatile ("s_waitcnt vmcnt(0)" : "+v"(wn[0]), "+v"(wn[1]), "+v"(wn[2]), "+v"(wn[3]) :: "memory");
      static_assert (AG1_R == 4, "asm operand list");
      u64 w[AG1_R];
#pragma unroll
      for (int r = 0; r < AG1_R; r++) w[r] = wn[r];
      const u32 valid = vn;
      b_next = next_batch ();
      fetch (b_next);
      // Table protocol.  Slots come in aligned pairs read with one 16-byte LDS load; a key's probe chain is its home
      // pair, the next pair, ... and it lives in the first slot of the chain that was free when it arrived.  Almost
      // every record finds its key with that one load and adds to its counter (no compare-and-swap: a bucket holds
      // each key hundreds of times).  A new key is CASed into the first free slot of the chain while the table is
      // open; once it is closed (enough keys; a lane looks before each claim, so at most one more key per lane gets
      // in) that slot is MARKed instead, and a MARK ends the chain for everybody: either the key or a MARK wins the
      // slot, so a key is in the table for all of its records or for none (those go back to the bucket's front).
      // Lanes work through their unsettled records independently (a wave loops until all its lanes are through): the
      // iterations of a wave follow the lane with the most probes in total, not the worst probe of every record.
      {
        auto home = [] (u64 key) {
          u32 h = (u32) key ^ __builtin_amdgcn_alignbit ((u32) (key >> 32), (u32) (key >> 32), 17);
          h *= 0x9E3779B1u; h ^= h >> 15;
          return h & (AG1_S / 2 - 1);
        };
        // first, every record looks at its home pair (straight-line code: the four loads are in flight together) --
        // that settles all but a few per cent of them
        // (the loads are for every lane -- a slot without a record holds 0, whose home pair is as good as any -- and their
        // results pass through an asm statement: left alone the compiler reads the pair's first slot, waits, looks, and
        // reads the second slot inside a branch, record after record: eight LDS round trips in a row instead of one)
        u32 todo = 0;
        u32 hp[AG1_R];
        ulonglong2 hk[AG1_R];
#pragma unroll
        for (int r = 0; r < AG1_R; r++) {
          hp[r] = home (w[r] & R1_KEY_MASK);
          hk[r] = *reinterpret_cast<const ulonglong2 *> (&L.key[2 * hp[r]]);
        }
        asm volatile ("" : "+v"(hk[0].x), "+v"(hk[0].y), "+v"(hk[1].x), "+v"(hk[1].y), "+v"(hk[2].x), "+v"(hk[2].y), "+v"(hk[3].x), "+v"(hk[3].y));
#pragma unroll
        for (int r = 0; r < AG1_R; r++) {
          const u64 cur = w[r];
          if (((valid >> r) & 1u) && ((cur >> R1_FLAG_SHIFT) & 3ull) != 3ull) {
            const u64 key = cur & R1_KEY_MASK;
            const bool hx = hk[r].x == key, hy = hk[r].y == key;
            if (hx | hy) atomicAdd (&L.cnt[4 * hp[r] + (hx ? 0u : 2u) + ((u32) (cur >> (R1_FLAG_SHIFT + 1)) & 1u)], 1u);
            else todo |= 1u << r;
          }
        }
        // the rest (new keys, collisions, a closed table) one probe at a time, every lane through its own records
        u32 probes = 0;
        u32 r = todo ? (u32) __ffs ((int) todo) - 1u : 0u;
        u64 cur = (r == 0u) ? w[0] : (r == 1u) ? w[1] : (r == 2u) ? w[2] : w[3];
        u32 pair = home (cur & R1_KEY_MASK);
        while (todo) {
          bool adv = false, left = false;
          {
            const u64 key = cur & R1_KEY_MASK;
            const u32 strand = (u32) (cur >> (R1_FLAG_SHIFT + 1)) & 1u;
            const ulonglong2 kk = *reinterpret_cast<const ulonglong2 *> (&L.key[2 * pair]);
            if (kk.x == key || kk.y == key) { atomicAdd (&L.cnt[4 * pair + (kk.x == key ? 0u : 2u) + strand], 1u); adv = true; }
            else {
              const bool e0 = (kk.x == 0ull) | (kk.x == AG1_MARK), e1 = (kk.y == 0ull) | (kk.y == AG1_MARK);
              if (e0 | e1) {                            // the chain ends in this pair
                const u32 slot = 2 * pair + (e0 ? 0u : 1u);
                if ((e0 ? kk.x : kk.y) == AG1_MARK) { left = true; adv = true; }
                else {
                  const bool closed = __hip_atomic_load (&L.n_claimed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) > AG1_CLOSE_AT;
                  const u64 old = atomicCAS ((unsigned long long *) &L.key[slot], 0ull, closed ? AG1_MARK : (unsigned long long) key);
                  if (old == 0ull) {
                    if (closed) left = true;
                    else { atomicAdd (&L.n_claimed, 1u); atomicAdd (&L.cnt[2 * slot + strand], 1u); }
                    adv = true;
                  }                                     // else somebody else took the slot: look at the pair again
                }
              }
              else if (++probes >= AG1_S / 2) { left = true; adv = true; }   // every slot holds another key
              else pair = (pair + 1u) & (AG1_S / 2 - 1);
            }
          }
          if (left) {                                   // to the second pool (chunk ids from LDS)
            const u32 o = atomicAdd (&L.n_ovf, 1u);
            const u32 j = chunk_of_pos (BK, o), oc = chunk_id (j);
            if (oc != TJ_NOCHUNK) dst[(((u64) oc * TJ_CH0) << BK.ch_shift) + (o - ((j * TJ_CH0) << BK.ch_shift))] = cur;
          }
          if (adv) {
            todo &= todo - 1u; probes = 0;
            if (todo) {
              r = (u32) __ffs ((int) todo) - 1u;
              cur = (r == 1u) ? w[1] : (r == 2u) ? w[2] : w[3];
              pair = home (cur & R1_KEY_MASK);
            }
          }
        }
      }
    }
    __syncthreads ();

    u32 mine = 0;
    u64 metas[AG1_S / AG_BLOCK];
#pragma unroll
    for (int r = 0; r < AG1_S / AG_BLOCK; r++) {
      const int slot = tid + r * AG_BLOCK;
      metas[r] = 0;
      if (L.key[slot] && L.key[slot] != AG1_MARK) {
        const u32 cf = L.cnt[2 * slot], cr = L.cnt[2 * slot + 1];
        const u64 flag = (cf ? 1ull : 0ull) | (cr ? 2ull : 0ull);
        const u64 cnt = ((u64) cf + (u64) cr) & 0xFFFFFull;
        const int scnt = (cnt & 0x80000ull) ? (int) cnt - 0x100000 : (int) cnt;
        if (remove_biased ? (flag == 3ull) : (scnt > 1)) {
          const u64 key = L.key[slot];                  // the record's fields (see pack_rec1)
          const u64 len10 = ((key >> 24) & 0xFFull) | (((key >> 56) & 3ull) << 8);
          metas[r] = ((key >> 58) & 1ull) | (len10 << TJ_META_LEN_SHIFT) | (cnt << TJ_META_COUNT_SHIFT) |
                     (0xffeull << TJ_META_MISM_SHIFT) | (flag << TJ_META_FLAG_SHIFT);
          mine++;
        }
      }
    }
    const u32 x = wave_inclusive_scan (mine);
    if (lane == 63) L.wsum[wave] = x;
    __syncthreads ();
    u32 wbase = 0, total = 0;
    for (int wv = 0; wv < AG_BLOCK / 64; wv++) { const u32 sm = L.wsum[wv]; if (wv < wave) wbase += sm; total += sm; }
    if (tid == 0) L.total = total ? atomicAdd (&fin->n_kept, total) : 0u;
    __syncthreads ();
    u64 at = (u64) L.total + wbase + x - mine;
#pragma unroll
    for (int r = 0; r < AG1_S / AG_BLOCK; r++)
      if (metas[r]) {
        const u64 key = L.key[tid + r * AG_BLOCK];
        if (at < kept_cap) {
          u64 *q = kept + 3 * at; q[0] = (key >> 32) & 0xFFFFFFull; q[1] = key & 0xFFFFFFull; q[2] = metas[r];
          if (fine) atomicAdd (&fine[bin_of_record ((key >> 32) & 0xFFFFFFull, key & 0xFFFFFFull, metas[r], k, fine_bits)], 1u);
        }
        else flag_kept_overflow (fin);
        at++;
      }
    __threadfence_block ();
    __syncthreads ();
    n = L.n_ovf;
    { const u64 *t = src; src = dst; dst = (u64 *) t; }
    __syncthreads ();
  }
  plan_tail (fin, k, plan_cap, plan);
}

// ---- W = 2 (k <= 28): word 0 of the record is never 0 and leaves bit 63 free, so it doubles as the slot's claim word:
// compare-and-swap 0 -> (word0 | PENDING), write word 1, then store word0.  A prober that meets its own word0 with
// PENDING set looks again; with it clear the second word is there to compare.  Same structure as aggregate1_kernel:
// records in flight per lane, read-first probing (a bucket holds each key many times), slots in aligned pairs read
// together (a probe chain is home pair, next pair, ...; a key lives in the first slot of the chain that was free when it
// arrived), a closed table MARKs the free slot at the end of a probe chain so that a key is in the table for all of its
// records or for none, leftovers go to the second pool, no barrier in the record loop.  6144 slots (144 KB of LDS with
// the counters): a bucket of the long-read configuration (4.6 k keys) fits one round, and at the usual 2-3 k keys the
// home pair settles nine records in ten.
#define AG2_S        6144
#define AG2_PAIRS    (AG2_S / 2)
#define AG2_CLOSE_AT 2560
                                        // (closing early pays: at 4.6 k keys per bucket -- the long-read configuration -- a table filled to 75 % costs more in probes than the second round costs in traffic)
#define AG2_R        4                   // records in flight per lane
#define AG2_VALID    (1ull << 63)        // set in the stored second key word (bits 61-63 of it are not key)
#define AG2_PENDING  (1ull << 63)
#define AG2_MARK     (1ull << 63)        // PENDING without a word0 (word0 always has bit 0 set)

struct Agg2Lds
{
  ulonglong2 kk[AG2_S];                 // x: claim word (record word 0), y: second key word | VALID
  u32 cnt[2 * AG2_S];                   // per slot: forward / reverse strand
  u32 chunk[AG_NCH];
  u32 n_claimed, n_ovf, total;
  u32 next_batch;                       // (see aggregate1_kernel: batches are handed to the waves as they come for one)
  u32 wsum[AG_BLOCK / 64];
};

__global__ __launch_bounds__ (AG_BLOCK)
void aggregate2_kernel (Buckets BK, u64 *ovf, int k, int remove_biased, u64 *__restrict__ kept, u64 kept_cap, FinCounts *fin,
                        long plan_cap, FinPlan *plan, u32 *__restrict__ fine, int fine_bits)
{
  __shared__ Agg2Lds L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32 bkt = blockIdx.x;
  u32 n = BK.cursors[bkt * TJ_CSTRIDE];
  const u64 m56 = (1ull << 56) - 1ull, fmask = ~(3ull << 61);
  if (n) for (u32 j = (u32) tid; j <= chunk_of_pos (BK, n - 1u) && j < AG_NCH; j += AG_BLOCK) L.chunk[j] = bucket_chunk_id (BK, bkt, j, false, nullptr);
  auto chunk_id = [&] (u32 j) { return j < AG_NCH ? L.chunk[j] : bucket_chunk_id (BK, bkt, j, false, nullptr); };
  const u64 *src = BK.pool;
  u64 *dst = ovf;

  while (n > 0) {
    for (int i = tid; i < AG2_S; i += AG_BLOCK) { L.kk[i] = make_ulonglong2 (0ull, 0ull); L.cnt[2 * i] = 0; L.cnt[2 * i + 1] = 0; }
    if (tid == 0) { L.n_claimed = 0; L.n_ovf = 0; L.next_batch = 0; }
    __syncthreads ();

    u64 wn[2 * AG2_R];
    u32 vn = 0;
    auto fetch = [&] (u32 b0) {                         // see aggregate1_kernel: a round lies in at most two chunks
      vn = 0;
#pragma unroll
      for (int r = 0; r < 2 * AG2_R; r++) wn[r] = 0;
      if (b0 >= n) return;
      const u32 ch = (u32) TJ_CH0 << BK.ch_shift;
      const u32 j0 = chunk_of_pos (BK, b0), bound = (j0 + 1u) * ch;
      const u32 c0 = chunk_id (j0), c1 = (bound < n) ? chunk_id (j0 + 1u) : TJ_NOCHUNK;
      const u64 off0 = (u64) c0 * ch - (u64) j0 * ch, off1 = (u64) c1 * ch - (u64) bound;
#pragma unroll
      for (int r = 0; r < AG2_R; r++) {
        const u32 idx = b0 + (u32) r * 64u + (u32) lane;
        const bool hi = idx >= bound;
        if (idx < n && (hi ? c1 : c0) != TJ_NOCHUNK) {
          const ulonglong2 v = *reinterpret_cast<const ulonglong2 *> (src + 2 * ((hi ? off1 : off0) + idx));
          vn |= 1u << r; wn[2 * r] = v.x; wn[2 * r + 1] = v.y;
        }
      }
    };
    auto next_batch = [&] () {
      u32 b = 0;
      if (lane == 0) b = atomicAdd (&L.next_batch, 1u);
      return batch_start ((u32) __builtin_amdgcn_readfirstlane ((int) b), n, 64u * AG2_R);
    };
    u32 b_next = next_batch ();
    fetch (b_next);
    while (b_next < n) {
      asm volatile ("s_waitcnt vmcnt(0)" : "+v"(wn[0]), "+v"(wn[1]), "+v"(wn[2]), "+v"(wn[3]), "+v"(wn[4]), "+v"(wn[5]), "+v"(wn[6]), "+v"(wn[7]) :: "memory");
      static_assert (AG2_R == 4, "asm operand list");
      u64 w[2 * AG2_R];
#pragma unroll
      for (int r = 0; r < 2 * AG2_R; r++) w[r] = wn[r];
      const u32 valid = vn;
      b_next = next_batch ();
      fetch (b_next);
      {
        auto home = [] (u64 a, u64 b) {                 // home pair of a key
          const u64 key1 = b & ~(3ull << 61);
          u32 h = (u32) a ^ __builtin_amdgcn_alignbit ((u32) (a >> 32), (u32) (a >> 32), 19) ^
                  __builtin_amdgcn_alignbit ((u32) key1, (u32) key1, 11) ^ __builtin_amdgcn_alignbit ((u32) (key1 >> 32), (u32) (key1 >> 32), 25);
          h *= 0x9E3779B1u; h ^= h >> 15;
          return __umulhi (h, (u32) AG2_PAIRS);
        };
        // the two slots of a pair, loaded together (atomic loads keep the LDS address space)
        auto load_pair = [&] (u32 pair, ulonglong2 &s0, ulonglong2 &s1) {
          s0.x = __hip_atomic_load ((unsigned long long *) &L.kk[2 * pair].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          s0.y = __hip_atomic_load ((unsigned long long *) &L.kk[2 * pair].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          s1.x = __hip_atomic_load ((unsigned long long *) &L.kk[2 * pair + 1].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          s1.y = __hip_atomic_load ((unsigned long long *) &L.kk[2 * pair + 1].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        };
        // First, every record walks the first pairs of its chain in straight-line code (the loads of all records of a
        // lane are in flight together): a published claim word with the record's own valid second word settles it, a full
        // pair of other keys sends it on to the next pair; anything else (a free slot: the key is new; a slot in the
        // middle of being published) is left to the general loop below, which starts at the pair reached here.
        u32 todo = 0, look = 0, cur[AG2_R];
#pragma unroll
        for (int q = 0; q < AG2_R; q++) {
          cur[q] = 0;
          if (((valid >> q) & 1u) && ((w[2 * q + 1] >> 61) & 3ull) != 3ull) { look |= 1u << q; cur[q] = home (w[2 * q], w[2 * q + 1]); }
        }
#pragma unroll
        for (int pass = 0; pass < 3; pass++) {
          if (pass && !look) break;
#pragma unroll
          for (int q = 0; q < AG2_R; q++)
            if ((look >> q) & 1u) {
              const u64 a0 = w[2 * q], a1 = w[2 * q + 1];
              ulonglong2 s0, s1;
              load_pair (cur[q], s0, s1);
              const u64 want = (a1 & fmask) | AG2_VALID;
              const bool m0 = (s0.x == a0) & (s0.y == want), m1 = (s1.x == a0) & (s1.y == want);
              if (m0 | m1) { atomicAdd (&L.cnt[2 * (2 * cur[q] + (m0 ? 0u : 1u)) + ((u32) (a1 >> 62) & 1u)], 1u); look &= ~(1u << q); }
              else {
                const u64 mine = a0 | AG2_PENDING;
                // (a slot holding another key: claim word published, not ours -- or ours with a valid second word that differs)
                const bool o0 = (s0.x != 0ull) & (s0.x != AG2_MARK) & (s0.x != mine) & ((s0.x & AG2_PENDING) == 0ull) & ((s0.x != a0) | ((s0.y & AG2_VALID) != 0ull));
                const bool o1 = (s1.x != 0ull) & (s1.x != AG2_MARK) & (s1.x != mine) & ((s1.x & AG2_PENDING) == 0ull) & ((s1.x != a0) | ((s1.y & AG2_VALID) != 0ull));
                if (o0 & o1) cur[q] = (cur[q] + 1u == (u32) AG2_PAIRS) ? 0u : cur[q] + 1u;
                else { look &= ~(1u << q); todo |= 1u << q; }
              }
            }
        }
        todo |= look;
        u32 probes = 0;
        u32 r = todo ? (u32) __ffs ((int) todo) - 1u : 0u;
        u64 w0 = (r == 0u) ? w[0] : (r == 1u) ? w[2] : (r == 2u) ? w[4] : w[6];
        u64 w1 = (r == 0u) ? w[1] : (r == 1u) ? w[3] : (r == 2u) ? w[5] : w[7];
        u32 pair = (r == 0u) ? cur[0] : (r == 1u) ? cur[1] : (r == 2u) ? cur[2] : cur[3];
        while (todo) {
          bool adv = false, left = false;
          {
            const u64 key1 = w1 & fmask, want = key1 | AG2_VALID;
            const u32 strand = (u32) (w1 >> 62) & 1u;
            ulonglong2 s0, s1;
            load_pair (pair, s0, s1);
            const bool m0 = (s0.x == w0) & (s0.y == want), m1 = (s1.x == w0) & (s1.y == want);
            // our own claim word still PENDING, or published next to a second word that is not valid yet (the loads
            // straddled the owner's writes): look at the pair again
            const bool again = (s0.x == (w0 | AG2_PENDING)) | (s1.x == (w0 | AG2_PENDING)) |
                               ((s0.x == w0) & !(s0.y & AG2_VALID)) | ((s1.x == w0) & !(s1.y & AG2_VALID));
            if (m0 | m1) { atomicAdd (&L.cnt[2 * (2 * pair + (m0 ? 0u : 1u)) + strand], 1u); adv = true; }
            else if (!again) {
              const bool e0 = (s0.x == 0ull) | (s0.x == AG2_MARK), e1 = (s1.x == 0ull) | (s1.x == AG2_MARK);
              if (e0 | e1) {                            // the chain ends in this pair
                const u32 slot = 2 * pair + (e0 ? 0u : 1u);
                if ((e0 ? s0.x : s1.x) == AG2_MARK) { left = true; adv = true; }
                else {                                  // claim the slot, or MARK it if the table is closed
                  const bool closed = __hip_atomic_load (&L.n_claimed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) > AG2_CLOSE_AT;
                  const u64 old = atomicCAS ((unsigned long long *) &L.kk[slot].x, 0ull, closed ? AG2_MARK : (unsigned long long) (w0 | AG2_PENDING));
                  if (old == 0ull) {
                    if (closed) left = true;
                    else {                              // claimed: publish the second word, then the first
                      __hip_atomic_store ((unsigned long long *) &L.kk[slot].y, (unsigned long long) want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                      atomicAdd (&L.n_claimed, 1u);
                      __hip_atomic_store ((unsigned long long *) &L.kk[slot].x, (unsigned long long) w0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                      atomicAdd (&L.cnt[2 * slot + strand], 1u);
                    }
                    adv = true;
                  }                                     // else somebody else took the slot: look at the pair again
                }
              }
              else if (++probes >= AG2_PAIRS) { left = true; adv = true; }   // every slot holds another key
              else pair = (pair + 1u == (u32) AG2_PAIRS) ? 0u : pair + 1u;
            }
          }
          if (left) {
            const u32 o = atomicAdd (&L.n_ovf, 1u);
            const u32 j = chunk_of_pos (BK, o), oc = chunk_id (j);
            if (oc != TJ_NOCHUNK) {
              const u64 at = (((u64) oc * TJ_CH0) << BK.ch_shift) + (o - ((j * TJ_CH0) << BK.ch_shift));
              dst[2 * at] = w0; dst[2 * at + 1] = w1;
            }
          }
          if (adv) {
            todo &= todo - 1u; probes = 0;
            if (todo) {
              r = (u32) __ffs ((int) todo) - 1u;
              w0 = (r == 1u) ? w[2] : (r == 2u) ? w[4] : w[6];
              w1 = (r == 1u) ? w[3] : (r == 2u) ? w[5] : w[7];
              pair = (r == 1u) ? cur[1] : (r == 2u) ? cur[2] : cur[3];
            }
          }
        }
      }
    }
    __syncthreads ();

    u32 mine = 0;
    u64 metas[AG2_S / AG_BLOCK];
#pragma unroll
    for (int r = 0; r < AG2_S / AG_BLOCK; r++) {
      const int slot = tid + r * AG_BLOCK;
      metas[r] = 0;
      if (L.kk[slot].x && L.kk[slot].x != AG2_MARK) {
        const u32 cf = L.cnt[2 * slot], cr = L.cnt[2 * slot + 1];
        const u64 flag = (cf ? 1ull : 0ull) | (cr ? 2ull : 0ull);
        const u64 cnt = ((u64) cf + (u64) cr) & 0xFFFFFull;
        const int scnt = (cnt & 0x80000ull) ? (int) cnt - 0x100000 : (int) cnt;
        if (remove_biased ? (flag == 3ull) : (scnt > 1)) {
          const u64 a = L.kk[slot].x, b = L.kk[slot].y;
          const u64 len10 = ((a >> 2) & 31ull) | (((b >> 56) & 31ull) << 5);
          metas[r] = ((a >> 1) & 1ull) | (len10 << TJ_META_LEN_SHIFT) | (cnt << TJ_META_COUNT_SHIFT) |
                     (0xffeull << TJ_META_MISM_SHIFT) | (flag << TJ_META_FLAG_SHIFT);
          mine++;
        }
      }
    }
    const u32 x = wave_inclusive_scan (mine);
    if (lane == 63) L.wsum[wave] = x;
    __syncthreads ();
    u32 wbase = 0, total = 0;
    for (int wv = 0; wv < AG_BLOCK / 64; wv++) { const u32 sm = L.wsum[wv]; if (wv < wave) wbase += sm; total += sm; }
    if (tid == 0) L.total = total ? atomicAdd (&fin->n_kept, total) : 0u;
    __syncthreads ();
    u64 at = (u64) L.total + wbase + x - mine;
#pragma unroll
    for (int r = 0; r < AG2_S / AG_BLOCK; r++)
      if (metas[r]) {
        const int slot = tid + r * AG_BLOCK;
        if (at < kept_cap) {
          u64 *q = kept + 3 * at; q[0] = (L.kk[slot].x >> 7) & m56; q[1] = L.kk[slot].y & m56; q[2] = metas[r];
          if (fine) atomicAdd (&fine[bin_of_record ((L.kk[slot].x >> 7) & m56, L.kk[slot].y & m56, metas[r], k, fine_bits)], 1u);
        }
        else flag_kept_overflow (fin);
        at++;
      }
    __threadfence_block ();
    __syncthreads ();
    n = L.n_ovf;
    { const u64 *t = src; src = dst; dst = (u64 *) t; }
    __syncthreads ();
  }
  plan_tail (fin, k, plan_cap, plan);
}

// ---- W = 4 (k <= 32): the k-mers fill their 64-bit words, so the claim word is made of the small key part and a hash:
// 1 | (base | length << 2) << 1 | 50 hash bits << 13 (never 0, bit 63 free).  Same protocol as aggregate2_kernel; a match
// needs the claim word AND both k-mers, and because the k-mer words have no room for a VALID bit, a claim-word match
// whose k-mers differ -- or are both 0, the cleared state -- is confirmed with a second look before it counts.
#define AG4_S        4096
#define AG4_CLOSE_AT 2560
#define AG4_R        2
#define AG4_PENDING  (1ull << 63)
#define AG4_MARK     (1ull << 63)

struct Agg4Lds
{
  u64 cw[AG4_S], c0[AG4_S], c1[AG4_S];
  u32 cnt[2 * AG4_S];
  u32 chunk[AG_NCH];
  u32 n_claimed, n_ovf, total;
  u32 next_batch;                       // (see aggregate1_kernel)
  u32 wsum[AG_BLOCK / 64];
};

__global__ __launch_bounds__ (AG_BLOCK)
void aggregate4_kernel (Buckets BK, u64 *ovf, int k, int remove_biased, u64 *__restrict__ kept, u64 kept_cap, FinCounts *fin,
                        long plan_cap, FinPlan *plan, u32 *__restrict__ fine, int fine_bits)
{
  __shared__ Agg4Lds L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32 bkt = blockIdx.x;
  u32 n = BK.cursors[bkt * TJ_CSTRIDE];
  if (n) for (u32 j = (u32) tid; j <= chunk_of_pos (BK, n - 1u) && j < AG_NCH; j += AG_BLOCK) L.chunk[j] = bucket_chunk_id (BK, bkt, j, false, nullptr);
  auto chunk_id = [&] (u32 j) { return j < AG_NCH ? L.chunk[j] : bucket_chunk_id (BK, bkt, j, false, nullptr); };
  const u64 *src = BK.pool;
  u64 *dst = ovf;
  auto ld = [] (u64 *p) { return (u64) __hip_atomic_load ((unsigned long long *) p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };

  while (n > 0) {
    for (int i = tid; i < AG4_S; i += AG_BLOCK) { L.cw[i] = 0; L.c0[i] = 0; L.c1[i] = 0; L.cnt[2 * i] = 0; L.cnt[2 * i + 1] = 0; }
    if (tid == 0) { L.n_claimed = 0; L.n_ovf = 0; L.next_batch = 0; }
    __syncthreads ();

    u64 wn[3 * AG4_R];                                  // (the fourth word of a record is padding)
    u32 vn = 0;
    auto fetch = [&] (u32 b0) {                         // see aggregate1_kernel: a round lies in at most two chunks
      vn = 0;
#pragma unroll
      for (int r = 0; r < 3 * AG4_R; r++) wn[r] = 0;
      if (b0 >= n) return;
      const u32 ch = (u32) TJ_CH0 << BK.ch_shift;
      const u32 j0 = chunk_of_pos (BK, b0), bound = (j0 + 1u) * ch;
      const u32 c0 = chunk_id (j0), c1 = (bound < n) ? chunk_id (j0 + 1u) : TJ_NOCHUNK;
      const u64 off0 = (u64) c0 * ch - (u64) j0 * ch, off1 = (u64) c1 * ch - (u64) bound;
#pragma unroll
      for (int r = 0; r < AG4_R; r++) {
        const u32 idx = b0 + (u32) r * 64u + (u32) lane;
        const bool hi = idx >= bound;
        if (idx < n && (hi ? c1 : c0) != TJ_NOCHUNK) {
          const u64 *p = src + 4 * ((hi ? off1 : off0) + idx);
          const ulonglong2 v = *reinterpret_cast<const ulonglong2 *> (p);
          vn |= 1u << r; wn[3 * r] = v.x; wn[3 * r + 1] = v.y; wn[3 * r + 2] = p[2];
        }
      }
    };
    auto next_batch = [&] () {
      u32 b = 0;
      if (lane == 0) b = atomicAdd (&L.next_batch, 1u);
      return batch_start ((u32) __builtin_amdgcn_readfirstlane ((int) b), n, 64u * AG4_R);
    };
    u32 b_next = next_batch ();
    fetch (b_next);
    while (b_next < n) {
      asm volatile ("s_waitcnt vmcnt(0)" : "+v"(wn[0]), "+v"(wn[1]), "+v"(wn[2]), "+v"(wn[3]), "+v"(wn[4]), "+v"(wn[5]) :: "memory");
      static_assert (AG4_R == 2, "asm operand list");
      u64 w[3 * AG4_R];
#pragma unroll
      for (int r = 0; r < 3 * AG4_R; r++) w[r] = wn[r];
      const u32 valid = vn;
      b_next = next_batch ();
      fetch (b_next);
      u32 todo = 0;
#pragma unroll
      for (int q = 0; q < AG4_R; q++) if (((valid >> q) & 1u) && ((w[3 * q + 2] >> 12) & 3ull) != 3ull) todo |= 1u << q;
      u32 probes = 0;
      while (todo) {
        const u32 r = (u32) __ffs ((int) todo) - 1u;
        const u64 c0 = r ? w[3] : w[0], c1 = r ? w[4] : w[1], m2 = r ? w[5] : w[2];
        const u32 k2 = (u32) m2 & 0xFFFu, strand = (u32) (m2 >> 13) & 1u;     // flag 1 = as read, 2 = reverse-complemented
        const u64 hk = hash_key (c0, c1, k2 & 3u, k2 >> 2);
        const u64 cw = 1ull | ((u64) k2 << 1) | ((hk >> 14) << 13);
        u32 slot = ((u32) hk + probes) & (AG4_S - 1);     // (linear probing: the probe count is the offset)
        bool adv = false, left = false;
        const u64 a = ld (&L.cw[slot]);
        u64 x0 = ld (&L.c0[slot]), x1 = ld (&L.c1[slot]);
        if (a == cw) {
          bool eq = (x0 == c0) & (x1 == c1);
          if (!eq || (c0 | c1) == 0ull) { x0 = ld (&L.c0[slot]); x1 = ld (&L.c1[slot]); eq = (x0 == c0) & (x1 == c1); }   // second look, after the claim word was seen published
          if (eq) { atomicAdd (&L.cnt[2 * slot + strand], 1u); adv = true; }
          else if (++probes >= AG4_S) { left = true; adv = true; }
        }
        else if (a == AG4_MARK) { left = true; adv = true; }
        else if (a == 0ull) {                           // the chain ends here: claim the slot, or MARK it if the table is closed
          const bool closed = __hip_atomic_load (&L.n_claimed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) > AG4_CLOSE_AT;
          const u64 old = atomicCAS ((unsigned long long *) &L.cw[slot], 0ull, closed ? AG4_MARK : (unsigned long long) (cw | AG4_PENDING));
          if (old == 0ull) {
            if (closed) left = true;
            else {                                      // claimed: publish the k-mers, then the claim word
              __hip_atomic_store ((unsigned long long *) &L.c0[slot], (unsigned long long) c0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              __hip_atomic_store ((unsigned long long *) &L.c1[slot], (unsigned long long) c1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              atomicAdd (&L.n_claimed, 1u);
              __hip_atomic_store ((unsigned long long *) &L.cw[slot], (unsigned long long) cw, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
              atomicAdd (&L.cnt[2 * slot + strand], 1u);
            }
            adv = true;
          }                                             // else somebody else took the slot: look at it again
        }
        else if (a != (cw | AG4_PENDING)) {             // another key (PENDING with our claim word: its owner is still writing, look again)
          if (++probes >= AG4_S) { left = true; adv = true; }
        }
        if (left) {
          const u32 o = atomicAdd (&L.n_ovf, 1u);
          const u32 j = chunk_of_pos (BK, o), oc = chunk_id (j);
          if (oc != TJ_NOCHUNK) {
            u64 *q = dst + 4 * ((((u64) oc * TJ_CH0) << BK.ch_shift) + (o - ((j * TJ_CH0) << BK.ch_shift)));
            q[0] = c0; q[1] = c1; q[2] = m2; q[3] = 0;
          }
        }
        if (adv) { todo &= todo - 1u; probes = 0; }
      }
    }
    __syncthreads ();

    u32 mine = 0;
    u64 metas[AG4_S / AG_BLOCK];
#pragma unroll
    for (int r = 0; r < AG4_S / AG_BLOCK; r++) {
      const int slot = tid + r * AG_BLOCK;
      metas[r] = 0;
      const u64 cw = L.cw[slot];
      if (cw && cw != AG4_MARK) {
        const u32 cf = L.cnt[2 * slot], cr = L.cnt[2 * slot + 1];
        const u64 flag = (cf ? 1ull : 0ull) | (cr ? 2ull : 0ull);
        const u64 cnt = ((u64) cf + (u64) cr) & 0xFFFFFull;           // 20-bit store wraps (reference :361)
        const int scnt = (cnt & 0x80000ull) ? (int) cnt - 0x100000 : (int) cnt;
        if (remove_biased ? (flag == 3ull) : (scnt > 1)) {
          const u32 k2 = (u32) (cw >> 1) & 0xFFFu;
          metas[r] = (u64) (k2 & 3u) | ((u64) (k2 >> 2) << TJ_META_LEN_SHIFT) | (cnt << TJ_META_COUNT_SHIFT) |
                     (0xffeull << TJ_META_MISM_SHIFT) | (flag << TJ_META_FLAG_SHIFT);
          mine++;
        }
      }
    }
    const u32 x = wave_inclusive_scan (mine);
    if (lane == 63) L.wsum[wave] = x;
    __syncthreads ();
    u32 wbase = 0, total = 0;
    for (int wv = 0; wv < AG_BLOCK / 64; wv++) { const u32 sm = L.wsum[wv]; if (wv < wave) wbase += sm; total += sm; }
    if (tid == 0) L.total = total ? atomicAdd (&fin->n_kept, total) : 0u;
    __syncthreads ();
    u64 at = (u64) L.total + wbase + x - mine;
#pragma unroll
    for (int r = 0; r < AG4_S / AG_BLOCK; r++)
      if (metas[r]) {
        const int slot = tid + r * AG_BLOCK;
        if (at < kept_cap) {
          u64 *q = kept + 3 * at; q[0] = L.c0[slot]; q[1] = L.c1[slot]; q[2] = metas[r];
          if (fine) atomicAdd (&fine[bin_of_record (L.c0[slot], L.c1[slot], metas[r], k, fine_bits)], 1u);
        }
        else flag_kept_overflow (fin);
        at++;
      }
    __threadfence_block ();
    __syncthreads ();
    n = L.n_ovf;
    { const u64 *t = src; src = dst; dst = (u64 *) t; }
    __syncthreads ();
  }
  plan_tail (fin, k, plan_cap, plan);
}

// ---------------------------------------------------------------------------------------------------------------
// sort key.  Reference order (src/hopo_counter.c:28-38): base, context[0], context[1], length, all descending, with
// length compared as a signed 10-bit value.  The strand flag is appended as the least significant digit so that the
// first and last member of a run of equal keys carry the OR of all flags.  The key is a bit string
//   [flag:2][length^0x200:10][ctx1:2k][ctx0:2k][base:1]   (least significant first), cut into 8-bit digits;
// the sort is an ascending LSD radix sort on the complemented digits.

__device__ __forceinline__ u32 key_digit (u64 c0, u64 c1, u64 meta, int pass, int k)
{
  const int o = 8 * pass;
  const u32 v12 = (u32) ((((meta >> TJ_META_LEN_SHIFT) & 0x3FFull) ^ 0x200ull) << 2) | (u32) ((meta >> TJ_META_FLAG_SHIFT) & 3ull);
  const u64 base = meta & 1ull;
  u32 d = 0;
  int lo;
  lo = o;                      if (lo < 12)                       d |= (u32) (v12 >> lo);
  lo = o - 12;                 if (lo < 2 * k && lo > -8)         d |= (u32) (lo >= 0 ? (c1 >> lo) : (c1 << -lo));
  lo = o - 12 - 2 * k;         if (lo < 2 * k && lo > -8)         d |= (u32) (lo >= 0 ? (c0 >> lo) : (c0 << -lo));
  lo = o - 12 - 4 * k;         if (lo < 1 && lo > -8)             d |= (u32) (base << -lo);
  return (~d) & 0xFFu;
}

__host__ int key_passes (int k) { return (13 + 4 * k + 7) / 8; }

#define RS_ITEMS      1024           // per workgroup: the sort only ever sees the kept set (1e5..1e6 records), so favour many small blocks
#define RS_WAVE_ITEMS 256

// lanes of the wavefront holding the same 8-bit digit as this lane
__device__ __forceinline__ u64 match_digit (u32 d, bool active)
{
  u64 peers = __ballot (active);
#pragma unroll
  for (int b = 0; b < 8; b++) {
    u64 bal = __ballot ((d >> b) & 1u);
    peers &= ((d >> b) & 1u) ? bal : ~bal;
  }
  return active ? peers : 0ull;
}

__global__ __launch_bounds__ (256)
void radix_count_kernel (const u64 *__restrict__ in, long n, int pass, int k, u32 *__restrict__ hist, int nblk)
{
  __shared__ u32 h[256];
  const int tid = threadIdx.x, lane = tid & 63;
  const u64 lt = (1ull << lane) - 1ull;
  h[tid] = 0;
  __syncthreads ();
  const long base = (long) blockIdx.x * RS_ITEMS;
  for (int i = tid; i < RS_ITEMS; i += 256) {            // uniform trip count: ballots are wave-wide
    long r = base + i;
    bool active = r < n;
    u32 d = 0;
    if (active) { const u64 *p = in + 3 * r; d = key_digit (p[0], p[1], p[2], pass, k); }
    u64 peers = match_digit (d, active);
    if (active && (peers & lt) == 0ull) atomicAdd (&h[d], (u32) __popcll (peers));   // one LDS atomic per distinct digit
  }
  __syncthreads ();
  hist[(long) tid * nblk + blockIdx.x] = h[tid];
}

__global__ __launch_bounds__ (256)
void radix_scatter_kernel (const u64 *__restrict__ in, u64 *__restrict__ out, long n, int pass, int k,
                           const u32 *__restrict__ offs, int nblk)
{
  __shared__ u32 wcnt[4][256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < 1024; i += 256) (&wcnt[0][0])[i] = 0;
  __syncthreads ();
  const long wbase = (long) blockIdx.x * RS_ITEMS + (long) wave * RS_WAVE_ITEMS;
  const u64 lt = (1ull << lane) - 1ull;

  for (int r = 0; r < RS_WAVE_ITEMS / 64; r++) {         // count this wave's digits
    long idx = wbase + r * 64 + lane;
    bool active = idx < n;
    u32 d = 0;
    if (active) { const u64 *p = in + 3 * idx; d = key_digit (p[0], p[1], p[2], pass, k); }
    u64 peers = match_digit (d, active);
    if (active && (peers & lt) == 0ull) atomicAdd (&wcnt[wave][d], (u32) __popcll (peers));
  }
  __syncthreads ();
  {                                                      // digit tid: global offset of each wave's first item
    u32 run = offs[(long) tid * nblk + blockIdx.x];
    for (int w = 0; w < 4; w++) { u32 c = wcnt[w][tid]; wcnt[w][tid] = run; run += c; }
  }
  __syncthreads ();
  for (int r = 0; r < RS_WAVE_ITEMS / 64; r++) {         // stable scatter, wave-synchronous
    long idx = wbase + r * 64 + lane;
    bool active = idx < n;
    u32 d = 0;
    u64 a = 0, b = 0, m = 0;
    if (active) { const u64 *p = in + 3 * idx; a = p[0]; b = p[1]; m = p[2]; d = key_digit (a, b, m, pass, k); }
    u64 peers = match_digit (d, active);
    int leader = active ? (__ffsll ((long long) peers) - 1) : 0;
    u32 old = 0;
    if (active && lane == leader) old = atomicAdd (&wcnt[wave][d], (u32) __popcll (peers));
    old = __shfl (old, leader);
    if (active) {
      u64 *q = out + 3 * ((u64) old + (u64) __popcll (peers & lt));
      q[0] = a; q[1] = b; q[2] = m;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Ordering the kept set (the usual case: 1e5..1e6 records, where seven stable radix passes are all launch overhead):
// one partition by the leading bits of the key into ~n/32 bins, then every bin is rank-sorted in LDS by one wavefront.
// Keys compare as the reference's qsort does (src/hopo_counter.c:28-38): base, ctx0, ctx1, signed length, descending.

#define BS_RANK_MAX  256                // records of one bin a wavefront sorts in LDS; a fuller bin -> radix sort instead

__device__ __forceinline__ u32 bin_of_record (u64 c0, u64 c1, u64 meta, int k, int nbits)
{ // leading nbits (<= 1 + 4k) of [base:1][ctx0:2k][ctx1:2k], complemented: ascending bins = descending keys
  const int kb = nbits - 1;
  const u64 v = (2 * k >= kb) ? (c0 >> (2 * k - kb)) : ((c0 << (kb - 2 * k)) | (c1 >> (4 * k - kb)));
  const u32 x = ((u32) (meta & 1ull) << kb) | (u32) v;
  return ((1u << nbits) - 1u) - x;
}

// does record a come before record b?  (equal keys -- only the merge ever has them -- keep their input order)
__device__ __forceinline__ bool record_before (u64 a0, u64 a1, u64 am, u32 ai, u64 b0, u64 b1, u64 bm, u32 bi)
{
  const u32 ab = (u32) am & 1u, bb = (u32) bm & 1u;
  if (ab != bb) return ab > bb;
  if (a0 != b0) return a0 > b0;
  if (a1 != b1) return a1 > b1;
  const u32 al = ((u32) (am >> TJ_META_LEN_SHIFT) & 0x3FFu) ^ 0x200u, bl = ((u32) (bm >> TJ_META_LEN_SHIFT) & 0x3FFu) ^ 0x200u;
  if (al != bl) return al > bl;
  return ai < bi;
}

// Sorted inputs (the merge: every sample's histogram is in key order) put a wavefront's 64 consecutive records into one or
// two bins, and the device's global-atomic rate (~24 G/s, whatever the addresses) is what these kernels run at: with
// `grouped` the lanes of a wavefront that share a bin send ONE atomic (peeling one distinct bin per round).
// Returns the lane's position in its bin (scatter) -- or nothing useful for a pure count.
__device__ __forceinline__ u32 bin_reserve (u32 *__restrict__ cursors, u32 bin, bool active, int grouped)
{
  if (!grouped) return active ? atomicAdd (&cursors[bin], 1u) : 0u;
  const int lane = threadIdx.x & 63;
  u64 todo = __ballot (active);
  u32 pos = 0;
  while (todo) {
    const int leader = __ffsll ((long long) todo) - 1;
    const u32 lb = (u32) __builtin_amdgcn_readlane ((int) bin, leader);
    const u64 grp = __ballot (active && bin == lb) & todo;
    u32 base = 0;
    if (lane == leader) base = atomicAdd (&cursors[lb], (u32) __popcll (grp));
    base = (u32) __builtin_amdgcn_readlane ((int) base, leader);
    if ((grp >> lane) & 1ull) pos = base + (u32) __popcll (grp & ((1ull << lane) - 1ull));
    todo &= ~grp;
  }
  return pos;
}

__global__ __launch_bounds__ (256)
void bin_count_kernel (const u64 *__restrict__ in, long n, int k, int nbits, u32 *__restrict__ bins, uint4 *__restrict__ cov, long cov_vec, int grouped,
                       const FinPlan *__restrict__ plan = nullptr)
{ // (also empties the coverage table, which the sort pass three launches later fills: 16 bytes per store)
  if (plan) { if (!plan->ok) return; n = plan->n1; nbits = plan->nbits; cov_vec = plan->t / 2; }
  for (long i = (long) blockIdx.x * 256 + threadIdx.x; i < cov_vec; i += (long) gridDim.x * 256) cov[i] = make_uint4 (0, 0, 0, 0);
  for (long i0 = (long) blockIdx.x * 256; i0 < n; i0 += (long) gridDim.x * 256) {     // (wave-uniform trip count: ballots inside)
    const long i = i0 + threadIdx.x;
    u32 bin = 0;
    if (i < n) { const u64 *p = in + 3 * i; bin = bin_of_record (p[0], p[1], p[2], k, nbits); }
    (void) bin_reserve (bins, bin, i < n, grouped);
  }
}

// Exclusive prefix of n values by one workgroup of WGS_THREADS threads, WGS_CHUNK at a time with a running carry: every
// thread holds WGS_PER contiguous words in registers (16-byte loads, in flight together), sums them, one scan over
// the threads' sums, and the thread writes its words' prefixes where it read the words.  Returns the total; vmax =
// largest value.
// Four wavefronts, a few words of LDS and (see ORDER_KERNEL) at most 32 registers: the ordering step's kernels are
// sized to start beside three resident workgroups of scan_fast_kernel<1, true>, which leave a CU one wavefront of 32
// registers per SIMD and 58 KB of LDS.  The kernel's time is a chain of round trips, much the same for four wavefronts
// as for sixteen.
#define BS_MAXBINS (1 << BS_MAXBITS)
#define WGS_THREADS 256
#define WGS_WAVES  (WGS_THREADS / 64)
#define WGS_PER    8                    // (sixteen: 39 registers, or scratch under the cap)
#define WGS_CHUNK  (WGS_THREADS * WGS_PER)
// A kernel of the ordering step's planned path: workgroups of four wavefronts at most, 32 registers at most (the
// attribute counts in pairs on a device whose vector and accumulation registers are one file: 16 states 32).  The
// compiler keeps to the cap by spilling if it must, so the cap alone proves nothing: tests/test_order_budget.py reads
// registers, scratch and LDS from the compiler's remarks.
#define ORDER_REGS   __attribute__ ((amdgpu_num_vgpr (16)))
#define ORDER_KERNEL __launch_bounds__ (256) ORDER_REGS

struct WgScanLds { u32 wsum[2][WGS_WAVES]; u32 vmax; };   // (the sums of odd and even chunks apart: one barrier per chunk)

__device__ __forceinline__ u32 wg_exclusive_scan (const u32 *__restrict__ in, int n_all, u32 *__restrict__ out, u32 *__restrict__ out2, WgScanLds &L, u32 &vmax)
{
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // (arrays that are not 16-byte material -- fewer than four bins, in practice: one thread, one word at a time)
  if ((((size_t) in | (size_t) out | (size_t) out2) & 15) != 0 || (n_all & 3) != 0) {
    u32 run = 0, mx = 0;
    if (tid == 0) {
      for (int i = 0; i < n_all; i++) { const u32 v = in[i]; out[i] = run; if (out2) out2[i] = run; run += v; mx = max (mx, v); }
      L.wsum[0][0] = run; L.vmax = mx;
    }
    __syncthreads ();
    vmax = L.vmax;
    return L.wsum[0][0];
  }
  if (tid == 0) L.vmax = 0;
  __syncthreads ();
  u32 carry = 0;
  int par = 0;
  for (int base = 0; base < n_all; base += WGS_CHUNK, par ^= 1) {
    const int i0 = base + tid * WGS_PER;
    uint4 v[WGS_PER / 4];
#pragma unroll
    for (int q = 0; q < WGS_PER / 4; q++) {                // (n_all is a multiple of four: a 16-byte piece is inside or outside)
      v[q] = make_uint4 (0, 0, 0, 0);
      if (i0 + 4 * q < n_all) v[q] = *reinterpret_cast<const uint4 *> (in + i0 + 4 * q);
    }
    u32 sum = 0, mx = 0;
#pragma unroll
    for (int q = 0; q < WGS_PER / 4; q++) { sum += v[q].x + v[q].y + v[q].z + v[q].w; mx = max (max (mx, max (v[q].x, v[q].y)), max (v[q].z, v[q].w)); }
    const u32 incl = wave_inclusive_scan (sum);
    if (lane == 63) L.wsum[par][wave] = incl;
    for (int o = 32; o > 0; o >>= 1) mx = max (mx, (u32) __shfl_down ((int) mx, o));
    if (lane == 0 && mx) atomicMax (&L.vmax, mx);
    __syncthreads ();
    u32 run = carry + incl - sum, total = 0;
    for (int w = 0; w < WGS_WAVES; w++) { const u32 x = L.wsum[par][w]; if (w < wave) run += x; total += x; }
#pragma unroll
    for (int q = 0; q < WGS_PER / 4; q++) {
      uint4 o;
      o.x = run; run += v[q].x; o.y = run; run += v[q].y; o.z = run; run += v[q].z; o.w = run; run += v[q].w;
      if (i0 + 4 * q < n_all) {
        *reinterpret_cast<uint4 *> (out + i0 + 4 * q) = o;
        if (out2) *reinterpret_cast<uint4 *> (out2 + i0 + 4 * q) = o;
      }
    }
    carry += total;
  }
  __syncthreads ();
  vmax = L.vmax;
  return carry;
}

// bin counts -> binstart[0..nbins] and the scatter cursors (bins[] itself); a bin above rank_max switches the whole
// sort to the radix path (flag in FinCounts).  full (where given): the list of fuller bins that bin_sort_index_kernel
// writes, emptied here.
__global__ ORDER_KERNEL
void bin_scan_kernel (u32 *__restrict__ bins, int nbins, u32 *__restrict__ binstart, u32 rank_max, FinCounts *fin, const FinPlan *__restrict__ plan = nullptr,
                      u32 *__restrict__ full = nullptr)
{
  __shared__ WgScanLds L;
  u32 vmax;
  if (plan) { if (!plan->ok) return; nbins = plan->nbins; }
  const u32 total = wg_exclusive_scan (bins, nbins, binstart, bins, L, vmax);
  if (threadIdx.x == 0) { binstart[nbins] = total; fin->sort_fallback = vmax > rank_max ? 1u : 0u; if (full) full[0] = 0u; }
}

__global__ __launch_bounds__ (256)
void bin_scatter_kernel (const u64 *__restrict__ in, u64 *__restrict__ out, long n, int k, int nbits, u32 *__restrict__ cursors,
                         const FinPlan *__restrict__ plan = nullptr, uint4 *__restrict__ cov = nullptr)
{
  if (plan) { if (!plan->ok) return; n = plan->n1; nbits = plan->nbits; }
  // (no bin_count_kernel ran, see finalise_binned: the coverage table, which the next launch fills, is emptied here)
  if (cov) for (long i = (long) blockIdx.x * 256 + threadIdx.x; i < plan->t / 2; i += (long) gridDim.x * 256) cov[i] = make_uint4 (0, 0, 0, 0);
  for (long i = (long) blockIdx.x * 256 + threadIdx.x; i < n; i += (long) gridDim.x * 256) {
    const u64 *p = in + 3 * i;
    const u64 a = p[0], b = p[1], m = p[2];
    u64 *q = out + 3 * (u64) atomicAdd (&cursors[bin_of_record (a, b, m, k, nbits)], 1u);
    q[0] = a; q[1] = b; q[2] = m;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// exclusive scan of u32 arrays (three-kernel, recursive on block sums)

#define SC_ITEMS 4096

// the sum of x over this lane and the lanes before it in the wavefront by six __shfl_up steps, for any type that adds (wave_inclusive_scan: the DPP form for u32)
template <class T> __device__ __forceinline__ T wave_inclusive_sum (T x, int lane)
{
  #pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const T v = __shfl_up (x, o); if (lane >= o) x += v; }
  return x;
}

__device__ __forceinline__ u32 block_exclusive_scan_256 (u32 v, u32 *s_tmp, u32 &total)
{ // exclusive scan of one value per thread over 256 threads
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32 x = wave_inclusive_sum (v, lane);
  if (lane == 63) s_tmp[wave] = x;
  __syncthreads ();
  u32 wbase = 0;
  for (int w = 0; w < wave; w++) wbase += s_tmp[w];
  total = s_tmp[0] + s_tmp[1] + s_tmp[2] + s_tmp[3];
  __syncthreads ();
  return wbase + x - v;
}

// the sum of `mine` over the threads before this one in a workgroup of 1024, and over all of them; one barrier.  wsum: 16 words
// that nobody reads or writes between the barrier before the call and the barrier after it
__device__ __forceinline__ int block_exclusive_scan_1024 (int mine, int tid, int *wsum, int &total)
{
  const int lane = tid & 63, wave = tid >> 6;
  int incl = mine;                                      // (wave_inclusive_sum written out: through the helper the three kernels that scan here compile an instruction shorter, not to the same code)
  #pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up (incl, o);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads ();
  const int w = lane & 15;                              // every sixteen lanes hold the sixteen sums and fold them among themselves
  int all = wsum[w], before = w < wave ? all : 0;
  #pragma unroll
  for (int o = 1; o < 16; o <<= 1) { all += __shfl_xor (all, o); before += __shfl_xor (before, o); }
  total = all;
  return before + incl - mine;
}

__global__ __launch_bounds__ (256)
void scan_reduce_kernel (const u32 *__restrict__ in, long n, u32 *__restrict__ bsum)
{
  __shared__ u32 s_tmp[4];
  const long base = (long) blockIdx.x * SC_ITEMS + (long) threadIdx.x * 16;
  u32 s = 0;
  for (int i = 0; i < 16; i++) if (base + i < n) s += in[base + i];
  u32 total;
  block_exclusive_scan_256 (s, s_tmp, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__ (256)
void scan_apply_kernel (const u32 *__restrict__ in, u32 *__restrict__ out, long n, const u32 *__restrict__ boff, u32 *total_out)
{
  __shared__ u32 s_tmp[4];
  const long base = (long) blockIdx.x * SC_ITEMS + (long) threadIdx.x * 16;
  u32 v[16], s = 0;
  for (int i = 0; i < 16; i++) { v[i] = (base + i < n) ? in[base + i] : 0u; s += v[i]; }
  u32 total;
  u32 ex = block_exclusive_scan_256 (s, s_tmp, total) + (boff ? boff[blockIdx.x] : 0u);
  for (int i = 0; i < 16; i++) { if (base + i < n) out[base + i] = ex; ex += v[i]; }
  if (total_out && base <= n - 1 && n - 1 < base + 16) *total_out = ex;   // thread holding the last element
}

// ---------------------------------------------------------------------------------------------------------------
// reduce runs of equal keys (reference: src/hopo_counter.c:356-374), context index (:388-404), coverage (:419-438)

__device__ __forceinline__ bool same_key (const u64 *a, const u64 *b)
{ // base, context, length (not the flag, not the count)
  const u64 km = (3ull << TJ_META_BASE_SHIFT) | (0x3FFull << TJ_META_LEN_SHIFT);
  return a[0] == b[0] && a[1] == b[1] && ((a[2] ^ b[2]) & km) == 0ull;
}

__device__ __forceinline__ bool same_context (const u64 *a, const u64 *b)
{
  return a[0] == b[0] && a[1] == b[1] && ((a[2] ^ b[2]) & 3ull) == 0ull;
}

__device__ __forceinline__ int meta_count (u64 meta)
{ // signed 20-bit read-back
  int c = (int) ((meta >> TJ_META_COUNT_SHIFT) & 0xFFFFFull);
  return (c & 0x80000) ? c - 0x100000 : c;
}

__device__ __forceinline__ int meta_len (u64 meta)
{ // signed 10-bit read-back of the tract length
  int l = (int) ((meta >> TJ_META_LEN_SHIFT) & 0x3FFull);
  return (l & 0x200) ? l - 0x400 : l;
}

// rows i and j of a record array (three words a row) have the same context and base
__device__ __forceinline__ bool same_context_rows (const u64 *rec, long i, long j) { return same_context (rec + 3 * i, rec + 3 * j); }

__global__ void seg_heads_kernel (const u64 *__restrict__ rec, long n, u32 *__restrict__ flags, int context_only)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    bool head = (i == 0);
    if (!head) head = context_only ? !same_context (rec + 3 * i, rec + 3 * (i - 1)) : !same_key (rec + 3 * i, rec + 3 * (i - 1));
    flags[i] = head ? 1u : 0u;
  }
}

__global__ void seg_headpos_kernel (const u32 *__restrict__ flags, const u32 *__restrict__ segid, long n, u32 *__restrict__ headpos)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x)
    if (flags[i]) headpos[segid[i]] = (u32) i;
}

// one thread per context of the kept array: depth, index decision
__global__ void ctx_decide_kernel (const u64 *__restrict__ kept, long n1, const u32 *__restrict__ ctxpos, const u32 *n_ctx_p,
                                   int min_coverage, u32 *__restrict__ keep)
{
  const u32 n_ctx = *n_ctx_p;
  for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n_ctx; j += gridDim.x * blockDim.x) {
    const long s = ctxpos[j], e = (j + 1 < n_ctx) ? (long) ctxpos[j + 1] : n1;
    int depth = 0;
    for (long i = s; i < e; i++) depth += meta_count (kept[3 * i + 2]);
    keep[j] = depth >= min_coverage;
  }
}

__global__ void ctx_write_kernel (long n1, const u32 *__restrict__ ctxpos, const u32 *n_ctx_p, const u32 *__restrict__ keep,
                                  const u32 *__restrict__ outpos, int *__restrict__ idx_initial, int *__restrict__ idx_final)
{
  const u32 n_ctx = *n_ctx_p;
  for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n_ctx; j += gridDim.x * blockDim.x)
    if (keep[j]) {
      idx_initial[outpos[j]] = (int) ctxpos[j];
      idx_final[outpos[j]] = (j + 1 < n_ctx) ? (int) ctxpos[j + 1] : (int) n1;
    }
}

// coverage: pooled 31-bit-truncated flanks weighted by count, largest pooled weight wins (reference
// src/hopo_counter.c:419-438).  Open-addressing table in HBM, one 64-bit word per slot: key + 1 in the high half (0 =
// empty), the pooled weight in the low half.  A new key and its first weight go in with ONE compare-and-swap (the
// memory-side atomics are what this step runs at); a key that is already there gets a 32-bit add on the low half
// (wraps like the reference's int, never carries into the key).
__device__ __forceinline__ u64 cov_word (u32 key31, int w) { return ((u64) (key31 + 1u) << 32) | (u64) (u32) w; }

// The table addressed by the key itself (cov_plan_bits): one 64-bit add per flank.  The low half is the pooled weight (it
// wraps like the reference's int: the sum of sign-extended weights modulo 2^32); 2^33 per add keeps the high half
// non-zero for a key that was seen, whatever the weights' signs (|weight| < 2^30: a context's depth, the sum of at most
// 1024 counts of 20 bits), which is all that cov_max_part asks of it (and cannot wrap the word: a flank value is shared by
// at most 2 x 1024 records' both sides, far from 2^31 adds).
__device__ __forceinline__ void cov_direct_add (u32 key31, int w, u64 *__restrict__ tab)
{
  atomicAdd ((unsigned long long *) &tab[key31], (unsigned long long) (long long) w + (1ull << 33));
}

__device__ __forceinline__ void cov_add_from (u32 key31, u32 slot, int w, u64 *__restrict__ tab, int log2t)
{
  const u32 tmask = (1u << log2t) - 1u;
  for (u32 probe = 0; probe <= tmask; probe++) {
    const u64 old = atomicCAS ((unsigned long long *) &tab[slot], 0ull, (unsigned long long) cov_word (key31, w));
    if (old == 0ull) break;
    if ((u32) (old >> 32) == key31 + 1u) { atomicAdd (reinterpret_cast<u32 *> (&tab[slot]), (u32) w); break; }   // (little endian: low half first)
    slot = (slot + 1u) & tmask;
  }
}

__device__ __forceinline__ void cov_add (u32 key31, int w, u64 *__restrict__ tab, int log2t)
{
  cov_add_from (key31, (key31 * 2654435761u) >> (32 - log2t), w, tab, log2t);
}

// two keys at once: both compare-and-swaps are in flight together
__device__ __forceinline__ void cov_add2 (u32 ka, u32 kb, int w, u64 *__restrict__ tab, int log2t)
{
  const u32 tmask = (1u << log2t) - 1u;
  const u32 pa = (ka * 2654435761u) >> (32 - log2t), pb = (kb * 2654435761u) >> (32 - log2t);
  const u64 oa = atomicCAS ((unsigned long long *) &tab[pa], 0ull, (unsigned long long) cov_word (ka, w));
  const u64 ob = atomicCAS ((unsigned long long *) &tab[pb], 0ull, (unsigned long long) cov_word (kb, w));
  if (oa != 0ull) {
    if ((u32) (oa >> 32) == ka + 1u) atomicAdd (reinterpret_cast<u32 *> (&tab[pa]), (u32) w);
    else cov_add_from (ka, (pa + 1u) & tmask, w, tab, log2t);
  }
  // (both keys equal and the slot empty: the second compare-and-swap has seen the first one's word and adds to it)
  if (ob != 0ull) {
    if ((u32) (ob >> 32) == kb + 1u) atomicAdd (reinterpret_cast<u32 *> (&tab[pb]), (u32) w);
    else cov_add_from (kb, (pb + 1u) & tmask, w, tab, log2t);
  }
}

// the same in two halves, so that the caller can work while the two compare-and-swaps make their round trip to memory
__device__ __forceinline__ void cov_add2_issue (u32 ka, u32 kb, int w, u64 *__restrict__ tab, int log2t, u64 &oa, u64 &ob)
{
  const u32 pa = (ka * 2654435761u) >> (32 - log2t), pb = (kb * 2654435761u) >> (32 - log2t);
  oa = atomicCAS ((unsigned long long *) &tab[pa], 0ull, (unsigned long long) cov_word (ka, w));
  ob = atomicCAS ((unsigned long long *) &tab[pb], 0ull, (unsigned long long) cov_word (kb, w));
}
__device__ __forceinline__ void cov_add2_finish (u32 ka, u32 kb, int w, u64 *__restrict__ tab, int log2t, u64 oa, u64 ob)
{
  const u32 tmask = (1u << log2t) - 1u;
  const u32 pa = (ka * 2654435761u) >> (32 - log2t), pb = (kb * 2654435761u) >> (32 - log2t);
  if (oa != 0ull) {
    if ((u32) (oa >> 32) == ka + 1u) atomicAdd (reinterpret_cast<u32 *> (&tab[pa]), (u32) w);
    else cov_add_from (ka, (pa + 1u) & tmask, w, tab, log2t);
  }
  if (ob != 0ull) {
    if ((u32) (ob >> 32) == kb + 1u) atomicAdd (reinterpret_cast<u32 *> (&tab[pb]), (u32) w);
    else cov_add_from (kb, (pb + 1u) & tmask, w, tab, log2t);
  }
}

__global__ void cov_insert_kernel (const u64 *__restrict__ kept, long n1, u64 *__restrict__ tab, int log2t)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < 2 * n1; i += (long) gridDim.x * blockDim.x) {
    const long r = (i < n1) ? i : i - n1;
    cov_add ((u32) (kept[3 * r + (i < n1 ? 0 : 1)] & 0x7FFFFFFFull), meta_count (kept[3 * r + 2]), tab, log2t);
  }
}

// largest pooled weight of the table slice this workgroup looks at -> atomicMax (one atomic per workgroup)
__device__ __forceinline__ void cov_max_part (const u64 *__restrict__ tab, long t, int *result, int *s_best)
{
  int best = INT_MIN;
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < t; i += (long) gridDim.x * blockDim.x) {
    const u64 v = tab[i];
    if (v >> 32) best = max (best, (int) (u32) v);
  }
  for (int o = 32; o > 0; o >>= 1) best = max (best, __shfl_down (best, o));
  if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
  __syncthreads ();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int) blockDim.x / 64; w++) best = max (best, s_best[w]);
    if (best != INT_MIN) atomicMax (result, best);
  }
}

__global__ __launch_bounds__ (256)
void cov_max_kernel (const u64 *__restrict__ tab, long t, int *result)
{
  __shared__ int s_best[4];
  cov_max_part (tab, t, result, s_best);
}

// One wavefront per bin: the bin's records go to LDS, every lane counts the records that come before its own, and that
// rank is the record's place in the output -- plus everything else the finalise step needs from the sorted order: a
// context (base, ctx0, ctx1) never straddles bins (the bin is a prefix of it), so its depth, its first record and its
// size are all found among the bin's records -- and the coverage table takes the records in any order.
//   binctx[bin]        contexts of the bin that reach min_coverage
//   tstart/tend[st+o]  index range of the o-th such context of the bin (st = first record of the bin)
#define BSF_GRID 1024                   // workgroups of bin_sort_full_kernel (one wavefront each) at most

// the value that lane (lane ^ J) holds, without the LDS pipe: quad permutes for 1 and 2, a row shift either way for 4 and 8,
// gfx950's row and half swaps for 16 and 32 (a ds_bpermute per word and step kept the LDS pipe busy for half of the sort
// kernel's time: 168 of them per bin)
template <int J>
__device__ __forceinline__ u32 lane_xor (u32 v, int lane)
{
  if constexpr (J == 1) return (u32) __builtin_amdgcn_update_dpp (0, (int) v, 0xB1, 0xF, 0xF, false);        // quad_perm [1,0,3,2]
  else if constexpr (J == 2) return (u32) __builtin_amdgcn_update_dpp (0, (int) v, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
  else if constexpr (J == 4 || J == 8) {
    // (a bank is four lanes of a row: the banks whose lanes have bit J clear take the shift down from above, the others then
    // the shift up from below, into the same register -- no second value to choose from, which cost a register per word)
    constexpr int lo = J == 4 ? 0x5 : 0x3;
    const int up = __builtin_amdgcn_update_dpp (0, (int) v, 0x100 + J, 0xF, lo, false);                      // row_shl: lane i gets lane i + J
    return (u32) __builtin_amdgcn_update_dpp (up, (int) v, 0x110 + J, 0xF, 0xF ^ lo, false);                 // row_shr: lane i gets lane i - J
  }
  else if constexpr (J == 16) { const auto r = __builtin_amdgcn_permlane16_swap (v, v, false, false); return (lane & 16) ? r[0] : r[1]; }
  else { const auto r = __builtin_amdgcn_permlane32_swap (v, v, false, false); return (lane & 32) ? r[0] : r[1]; }
}

// Two kernels share this body, both within the ordering step's register budget (ORDER_KERNEL: one wavefront of 32
// registers per SIMD is what a CU full of scanning workgroups has left).  FULL = false, bin_sort_index_kernel: every bin
// in turn; a bin of at most 64 records is sorted across the lanes, a fuller one is only written to the list `full`
// (full[0]: how many, emptied by bin_scan_kernel; then the bins) -- as scan_fast_kernel lists its slow tiles -- because
// ranking it keeps much more alive than the sort does.  FULL = true, bin_sort_full_kernel, right behind on the same
// stream: the listed bins, ranked through LDS.
template <bool FULL>
__device__ __forceinline__ void bin_sort_index_bins (const u64 *__restrict__ in, u64 *__restrict__ out, const u32 *__restrict__ binstart, int nbins, const FinCounts *fin,
                                                     int min_coverage, u64 *__restrict__ cov_tab, int log2t,
                                                     u32 *__restrict__ binctx, u32 *__restrict__ tstart, u32 *__restrict__ tend, const FinPlan *__restrict__ plan,
                                                     int cov_direct, u32 *__restrict__ full, u32 *H, u32 *E)
{
  const int lane = threadIdx.x & 63;
  // (the first bin's bounds are asked for together with the plan: one round trip less in the chain; `nbins` as passed is
  // the layout's size, which the array has whatever the plan says)
  const int bin0 = (int) blockIdx.x;
  u32 st0 = 0, en0 = 0;
  if (!FULL && bin0 < nbins) { st0 = binstart[bin0]; en0 = binstart[bin0 + 1]; }
  if (plan) { if (!plan->ok) return; nbins = plan->nbins; log2t = plan->log2t; cov_direct = (int) plan->cov_direct; }
  if (fin->sort_fallback) return;                       // some bin is too full: the caller takes the radix path
  const u32 n_turns = FULL ? min (full[0], (u32) nbins) : (u32) nbins;
  for (u32 turn = blockIdx.x; turn < n_turns; turn += gridDim.x) {
    const int bin = FULL ? (int) full[1 + turn] : (int) turn;
    const u32 st = (!FULL && bin == bin0) ? st0 : binstart[bin], s = ((!FULL && bin == bin0) ? en0 : binstart[bin + 1]) - st;
    if (s == 0) { if (lane == 0) binctx[bin] = 0; continue; }
    const u64 *R = in + 3 * (u64) st;                   // the bin's records (a fuller bin reads them from here, the same record in every lane)
    u32 nkeep = 0;
    if constexpr (!FULL) {
      if (s <= 64u) {
        // the usual bin: sorted across the lanes, below
      }
      else { if (lane == 0) full[1u + atomicAdd (&full[0], 1u)] = (u32) bin; continue; }
      // The usual bin (a record per lane at most): a bitonic sort of the records across the wavefront's lanes -- 21
      // compare-and-exchange steps of some thirty instructions -- instead of every lane comparing its record with every
      // record of the bin (s / 4 turns of 180); sorted, a record's place is its lane, a context's records are neighbours,
      // and its size, depth and place among the contexts that are kept come out of two ballots and one prefix sum.
      const bool valid = (u32) lane < s;
      u64 a0 = 0, a1 = 0, am = 0;
      if (valid) { a0 = R[3 * lane]; a1 = R[3 * lane + 1]; am = R[3 * lane + 2]; }   // (one record per lane: its three loads are in flight together)
      // (a hashed coverage table: the record's two compare-and-swaps go out now and are looked at after the sort -- their round
      // trip to memory, a few microseconds, runs under it, and they stay with the lane that sent them.  Tried: reading the two
      // home slots first and adding where the key is already there, one atomic per flank instead of two -- no change, 177
      // against 179 us on the long-read sample: it is the random 8-byte accesses to a 64 MB table that this kernel waits for
      // there, whatever their kind)
      // (what outlives the sort of the record as it was loaded is its two 31-bit flanks and its count, three registers: the
      // kernel has 32 in all)
      const int w = meta_count (am);
      const u32 ka = (u32) a0 & 0x7FFFFFFFu, kb = (u32) a1 & 0x7FFFFFFFu;
      u64 cas_a = 0, cas_b = 0;
      if (!cov_direct && valid) cov_add2_issue (ka, kb, w, cov_tab, log2t, cas_a, cas_b);
      // order: records before empty lanes, then base, ctx0, ctx1, signed length, all descending (record_before); kh holds
      // what comes before the contexts, kl what comes after them (a lane's own number last: no two lanes compare equal)
      u32 kh = valid ? 2u | ((u32) am & 1u) : 0u;
      u32 kl = ((((u32) (am >> TJ_META_LEN_SHIFT) & 0x3FFu) ^ 0x200u) << 6) | (63u - (u32) lane);
      u32 x0 = (u32) a0, x1 = (u32) (a0 >> 32), y0 = (u32) a1, y1 = (u32) (a1 >> 32), m0 = (u32) am, m1 = (u32) (am >> 32);
      auto step = [&] (auto jc, int kk) {
        constexpr int J = decltype (jc)::value;
        const u32 ox0 = lane_xor<J> (x0, lane), ox1 = lane_xor<J> (x1, lane), oy0 = lane_xor<J> (y0, lane), oy1 = lane_xor<J> (y1, lane);
        const u32 om0 = lane_xor<J> (m0, lane), om1 = lane_xor<J> (m1, lane), okh = lane_xor<J> (kh, lane), okl = lane_xor<J> (kl, lane);
        const u64 mx = ((u64) x1 << 32) | x0, my = ((u64) y1 << 32) | y0, ox = ((u64) ox1 << 32) | ox0, oy = ((u64) oy1 << 32) | oy0;
        const bool mine_first = (kh > okh) | ((kh == okh) & ((mx > ox) | ((mx == ox) & ((my > oy) | ((my == oy) & (kl > okl))))));
        // the lower lane of a pair keeps the record that comes first where the run of kk lanes is to ascend, the other one where it is to descend
        const bool want_first = ((lane & kk) == 0) == ((lane & J) == 0);
        const bool take = mine_first != want_first;       // the partner's record
        x0 = take ? ox0 : x0; x1 = take ? ox1 : x1; y0 = take ? oy0 : y0; y1 = take ? oy1 : y1;
        m0 = take ? om0 : m0; m1 = take ? om1 : m1; kh = take ? okh : kh; kl = take ? okl : kl;
      };
#pragma unroll
      for (int kk = 2; kk <= 64; kk <<= 1) {
        if (kk >= 64) step (std::integral_constant<int, 32> (), kk);
        if (kk >= 32) step (std::integral_constant<int, 16> (), kk);
        if (kk >= 16) step (std::integral_constant<int, 8> (), kk);
        if (kk >= 8) step (std::integral_constant<int, 4> (), kk);
        if (kk >= 4) step (std::integral_constant<int, 2> (), kk);
        step (std::integral_constant<int, 1> (), kk);
      }
      // lane i holds the i-th record of the bin
      const bool have = kh >= 2u;                          // (the records are in lanes 0 .. s - 1 again)
      const u64 b0 = ((u64) x1 << 32) | x0, b1 = ((u64) y1 << 32) | y0, bm = ((u64) m1 << 32) | m0;
      if (have) { u64 *q = out + 3 * ((u64) st + (u32) lane); q[0] = b0; q[1] = b1; q[2] = bm; }
      // a context's first record: the lane before holds another context (or it is lane 0)
      const u32 px0 = (u32) __builtin_amdgcn_update_dpp (0, (int) x0, 0x138, 0xF, 0xF, false), px1 = (u32) __builtin_amdgcn_update_dpp (0, (int) x1, 0x138, 0xF, 0xF, false);
      const u32 py0 = (u32) __builtin_amdgcn_update_dpp (0, (int) y0, 0x138, 0xF, 0xF, false), py1 = (u32) __builtin_amdgcn_update_dpp (0, (int) y1, 0x138, 0xF, 0xF, false);
      const u32 pkh = (u32) __builtin_amdgcn_update_dpp (0, (int) kh, 0x138, 0xF, 0xF, false);
      const bool head = have & ((lane == 0) | (px0 != x0) | (px1 != x1) | (py0 != y0) | (py1 != y1) | (pkh != kh));
      const u64 heads = __ballot (head);
      const int cnt = have ? meta_count (bm) : 0;
      const u32 incl = wave_inclusive_scan ((u32) cnt);    // (wraps like the int sum it stands for)
      const u64 above = (lane == 63) ? 0ull : (heads >> (lane + 1));
      const u32 next_head = above ? (u32) lane + (u32) __ffsll ((long long) above) : s;   // first lane of the next context (or the end)
      const u32 last_incl = (u32) __builtin_amdgcn_ds_bpermute ((int) ((next_head - 1u) << 2), (int) incl);
      const int depth = (int) (last_incl - (incl - (u32) cnt));
      const bool keep = head & (depth >= min_coverage);
      const u64 keeps = __ballot (keep);
      if (keep) {
        const u32 o = (u32) __popcll (keeps & ((1ull << lane) - 1ull));
        tstart[st + o] = st + (u32) lane;
        tend[st + o] = st + next_head;
      }
      nkeep = (u32) __popcll (keeps);
      // The coverage table takes a context's records in one go: they pool under the same two flanks, so the context's depth
      // is added once for each (the sum of the counts, wrapping like the reference's int, whatever the order) -- the
      // memory-side atomics are what this kernel runs at (24 G/s whatever the addresses: 470 k adds were 20 of its 31 us on
      // the headline sample), and a context has 2.3 records on average.
      // (only where the table is addressed by the flank itself: a plain add needs no answer)
      if (cov_direct) {
        if (head) { cov_direct_add ((u32) (b0 & 0x7FFFFFFFull), depth, cov_tab); cov_direct_add ((u32) (b1 & 0x7FFFFFFFull), depth, cov_tab); }
      }
      else if (valid) {
        asm volatile ("" : "+v"(cas_a), "+v"(cas_b));      // (or the compiler tests them for zero, and waits, ahead of the sort)
        cov_add2_finish (ka, kb, w, cov_tab, log2t, cas_a, cas_b);
      }
      if (lane == 0) binctx[bin] = nkeep;
      asm volatile ("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier ();
      continue;
    }
    for (u32 t0 = 0; t0 < s; t0 += 64) {                  // (FULL only: the other kernel has listed the bin and gone on)
      const u32 t = t0 + lane;
      bool keep = false;
      if (t < s) {
        const u64 a0 = R[3 * t], a1 = R[3 * t + 1], am = R[3 * t + 2];
        u32 rank = 0, ctx_before = 0, ctx_size = 0;
        int depth = 0;
        // (the bin's records four at a time, the same for every lane: twelve LDS reads in flight for one wait, and the
        // comparison -- record_before, spelt without branches -- is a chain of lane masks: as nested ifs, one record per turn,
        // it was four exec regions and a wait for the reads in every turn, 220 cycles for 30 instructions)
        const u32 abase = (u32) am & 1u, alen = ((u32) (am >> TJ_META_LEN_SHIFT) & 0x3FFu) ^ 0x200u;
        for (u32 j0 = 0; j0 < s; j0 += 4) {
          u64 b0[4], b1[4], bm[4];
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const u32 jj = (j0 + (u32) i < s) ? j0 + (u32) i : s - 1u;
            b0[i] = R[3 * jj]; b1[i] = R[3 * jj + 1]; bm[i] = R[3 * jj + 2];
          }
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const u32 j = j0 + (u32) i;
            const bool live = j < s;                        // (uniform)
            const u32 bbase = (u32) bm[i] & 1u, blen = ((u32) (bm[i] >> TJ_META_LEN_SHIFT) & 0x3FFu) ^ 0x200u;
            const bool e0 = b0[i] == a0, e1 = b1[i] == a1, eb = bbase == abase;
            const bool before = live & ((bbase > abase) | (eb & ((b0[i] > a0) | (e0 & ((b1[i] > a1) | (e1 & ((blen > alen) | ((blen == alen) & (j < t)))))))));
            const bool same = live & e0 & e1 & (((u32) (bm[i] ^ am) & 3u) == 0u);
            rank += before ? 1u : 0u;
            ctx_size += same ? 1u : 0u;
            depth += same ? meta_count (bm[i]) : 0;
            ctx_before += (same & before) ? 1u : 0u;
          }
        }
        u64 *q = out + 3 * ((u64) st + rank);
        q[0] = a0; q[1] = a1; q[2] = am;
        keep = (ctx_before == 0u) && depth >= min_coverage;      // first record of its context, context deep enough
        H[t] = rank | (keep ? 0x80000000u : 0u);
        E[t] = ctx_size;
        if (ctx_before == 0u) {                            // (the context's depth, once for each flank: see above)
          if (cov_direct) { cov_direct_add ((u32) (a0 & 0x7FFFFFFFull), depth, cov_tab); cov_direct_add ((u32) (a1 & 0x7FFFFFFFull), depth, cov_tab); }
          else cov_add2 ((u32) (a0 & 0x7FFFFFFFull), (u32) (a1 & 0x7FFFFFFFull), depth, cov_tab, log2t);
        }
      }
      nkeep += (u32) __popcll (__ballot (keep));
    }
    asm volatile ("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier ();
    for (u32 t = lane; t < s; t += 64) {
      const u32 h = H[t];
      if (h & 0x80000000u) {
        const u32 rank = h & 0x7FFFFFFFu;
        u32 o = 0;
        for (u32 j = 0; j < s; j += 4) {                  // (four entries per LDS read; entries past the bin's end hold an earlier bin's)
          const uint4 g = *reinterpret_cast<const uint4 *> (&H[j]);
          o += ((g.x & 0x80000000u) && (g.x & 0x7FFFFFFFu) < rank) ? 1u : 0u;
          o += (j + 1u < s && (g.y & 0x80000000u) && (g.y & 0x7FFFFFFFu) < rank) ? 1u : 0u;
          o += (j + 2u < s && (g.z & 0x80000000u) && (g.z & 0x7FFFFFFFu) < rank) ? 1u : 0u;
          o += (j + 3u < s && (g.w & 0x80000000u) && (g.w & 0x7FFFFFFFu) < rank) ? 1u : 0u;
        }
        tstart[st + o] = st + rank;
        tend[st + o] = st + rank + E[t];
      }
    }
    if (lane == 0) binctx[bin] = nkeep;
    asm volatile ("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier ();
  }
}

__global__ __launch_bounds__ (64) ORDER_REGS
void bin_sort_index_kernel (const u64 *__restrict__ in, u64 *__restrict__ out, const u32 *__restrict__ binstart, int nbins, const FinCounts *fin,
                            int min_coverage, u64 *__restrict__ cov_tab, int log2t,
                            u32 *__restrict__ binctx, u32 *__restrict__ tstart, u32 *__restrict__ tend, u32 *__restrict__ full,
                            const FinPlan *__restrict__ plan = nullptr, int cov_direct = 0)
{
  bin_sort_index_bins<false> (in, out, binstart, nbins, fin, min_coverage, cov_tab, log2t, binctx, tstart, tend, plan, cov_direct, full, nullptr, nullptr);
}

__global__ __launch_bounds__ (64) ORDER_REGS
void bin_sort_full_kernel (const u64 *__restrict__ in, u64 *__restrict__ out, const u32 *__restrict__ binstart, int nbins, const FinCounts *fin,
                           int min_coverage, u64 *__restrict__ cov_tab, int log2t,
                           u32 *__restrict__ binctx, u32 *__restrict__ tstart, u32 *__restrict__ tend, u32 *__restrict__ full,
                           const FinPlan *__restrict__ plan = nullptr, int cov_direct = 0)
{
  // (2 KB of LDS: a bin's records are read where they lie, the same record in every lane -- with the records of up to 256
  // staged in LDS, 8 KB, fewer wavefronts fitted a CU, and a wavefront's time is a chain of memory round trips that only
  // other wavefronts can fill)
  __shared__ alignas (16) u32 hd[BS_RANK_MAX];
  __shared__ u32 sz[BS_RANK_MAX];
  bin_sort_index_bins<true> (in, out, binstart, nbins, fin, min_coverage, cov_tab, log2t, binctx, tstart, tend, plan, cov_direct, full, hd, sz);
}

// one workgroup: exclusive prefix of binctx -> binout, number of index ranges, coverage start value
__global__ ORDER_KERNEL
void bin_ctx_scan_kernel (const u32 *__restrict__ binctx, int nbins, u32 *__restrict__ binout, FinCounts *fin, const FinPlan *__restrict__ plan = nullptr)
{
  __shared__ WgScanLds L;
  u32 vmax;
  if (plan) { if (!plan->ok) return; nbins = plan->nbins; }
  const u32 total = wg_exclusive_scan (binctx, nbins, binout, nullptr, L, vmax);
  if (threadIdx.x == 0 && !fin->sort_fallback) { fin->n_idx = total; fin->coverage = INT_MIN; }
}

// index ranges in order (reference: idx_initial / idx_final, src/hopo_counter.c:388-404) + the coverage maximum
__global__ ORDER_KERNEL
void bin_ctx_write_kernel (const u32 *__restrict__ binstart, const u32 *__restrict__ binctx, const u32 *__restrict__ binout, int nbins,
                           const u32 *__restrict__ tstart, const u32 *__restrict__ tend, int *__restrict__ idx_initial, int *__restrict__ idx_final,
                           const u64 *__restrict__ cov_tab, long t, FinCounts *fin, const FinPlan *__restrict__ plan = nullptr)
{
  __shared__ int s_best[4];
  if (plan) { if (!plan->ok) return; nbins = plan->nbins; t = plan->t; }
  if (fin->sort_fallback) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int bin = blockIdx.x * 4 + wave; bin < nbins; bin += gridDim.x * 4) {
    const u32 cnt = binctx[bin], st = binstart[bin], o0 = binout[bin];
#pragma unroll 1
    for (u32 o = lane; o < cnt; o += 64) { idx_initial[o0 + o] = (int) tstart[st + o]; idx_final[o0 + o] = (int) tend[st + o]; }
  }
  // (cov_max_part with 32-bit indices -- a table has 2^31 slots at most, see cov_table_bits -- two slots per load and a fixed
  // unroll: written over `long` with the launch's sizes the loop cost 38 registers, six more than the ordering step's budget)
  int best = INT_MIN;
  const uint4 *tab2 = reinterpret_cast<const uint4 *> (cov_tab);
  const u32 half = (u32) (t >> 1);                       // (t is a power of two, 1024 at least)
#pragma unroll 2
  for (u32 i = blockIdx.x * 256u + threadIdx.x; i < half; i += gridDim.x * 256u) {
    const uint4 v = tab2[i];
    if (v.y) best = max (best, (int) v.x);
    if (v.w) best = max (best, (int) v.z);
  }
  for (int o = 32; o > 0; o >>= 1) best = max (best, __shfl_down (best, o));
  if (lane == 0) s_best[wave] = best;
  __syncthreads ();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) best = max (best, s_best[w]);
    if (best != INT_MIN) atomicMax (&fin->coverage, best);
  }
}

// ---- cross-sample merge on the bins --------------------------------------------------------------------------------
// The samples' histograms, back to back, are partitioned by the same leading key bits; one wavefront per bin then finds
// the distinct keys of its bin (the lowest-numbered record of each key represents it), their order, and the depth of
// each key over all samples.  MG_RANK_MAX bounds a bin (a fuller one -> radix path).
#define MG_RANK_MAX 256
#define TJ_META_SAMPLE_SHIFT 52          // bits 52..63 of the bitfield word are unused by hopo_element

__global__ __launch_bounds__ (256)
void merge_scatter_kernel (const u64 *__restrict__ in, u64 *__restrict__ out, long n, int k, int nbits, u32 *__restrict__ cursors,
                           const long *__restrict__ starts, int n_samples)
{ // bin_scatter_kernel + the sample index of every record written into the spare bits of its meta word
  for (long i0 = (long) blockIdx.x * 256; i0 < n; i0 += (long) gridDim.x * 256) {
    const long i = i0 + threadIdx.x;
    const bool active = i < n;
    u64 a = 0, b = 0, m = 0;
    int lo = 0;
    if (active) {
      int hi = n_samples;                               // starts[s] <= i < starts[s + 1]
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (starts[mid] <= i) lo = mid; else hi = mid; }
      const u64 *p = in + 3 * i;
      a = p[0]; b = p[1]; m = p[2];
    }
    const u32 pos = bin_reserve (cursors, active ? bin_of_record (a, b, m, k, nbits) : 0u, active, 1);
    if (active) {
      u64 *q = out + 3 * (u64) pos;
      q[0] = a; q[1] = b; q[2] = (m & ((1ull << TJ_META_SAMPLE_SHIFT) - 1ull)) | ((u64) lo << TJ_META_SAMPLE_SHIFT);
    }
  }
}

__device__ __forceinline__ bool merge_same_key (u64 a0, u64 a1, u64 am, u64 b0, u64 b1, u64 bm)
{
  const u64 km = (3ull << TJ_META_BASE_SHIFT) | (0x3FFull << TJ_META_LEN_SHIFT);
  return a0 == b0 && a1 == b1 && ((am ^ bm) & km) == 0ull;
}

// per bin: binctx[bin] = distinct keys; per record (at its place st + t in the partitioned array): tpos = rank of its
// key among the bin's distinct keys, ttot = depth of the key over all samples if the record represents its key, else ~0.
// Inside a bin the base is the same (it is the bin's leading bit), so keys compare as (ctx0, ctx1, length ^ 0x200).
__global__ __launch_bounds__ (64)
void bin_merge_kernel (const u64 *__restrict__ rec, const u32 *__restrict__ binstart, int nbins, const FinCounts *fin,
                       u32 *__restrict__ binctx, u32 *__restrict__ tpos, u32 *__restrict__ ttot)
{
  __shared__ u64 R[3 * MG_RANK_MAX];
  __shared__ alignas (16) u32 H[MG_RANK_MAX];           // records in front of this one's key | representative << 31
  if (fin->sort_fallback) return;
  const int lane = threadIdx.x;
  for (int bin = blockIdx.x; bin < nbins; bin += gridDim.x) {
    const u32 st = binstart[bin], s = binstart[bin + 1] - st;
    if (s == 0) { if (lane == 0) binctx[bin] = 0; continue; }
    for (u32 t = lane; t < s; t += 64) {                // one record per lane: its three loads are in flight together
      const u64 *p = rec + 3 * (u64) (st + t);
      const u64 v0 = p[0], v1 = p[1], v2 = p[2];
      R[3 * t] = v0; R[3 * t + 1] = v1;
      R[3 * t + 2] = (v2 & ~(0x3FFull << TJ_META_LEN_SHIFT)) | ((((v2 >> TJ_META_LEN_SHIFT) & 0x3FFull) ^ 0x200ull) << TJ_META_LEN_SHIFT);   // length as an unsigned sort key
    }
    asm volatile ("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier ();
    const u64 lmask = 0x3FFull << TJ_META_LEN_SHIFT;
    u32 nrep = 0;
    for (u32 t0 = 0; t0 < s; t0 += 64) {                // pass 1: records in front, who represents its key, the key's depth
      const u32 t = t0 + lane;
      bool rep = false;
      if (t < s) {
        const u64 a0 = R[3 * t], a1 = R[3 * t + 1], al = R[3 * t + 2] & lmask;
        rep = true;
        u32 tot = 0, r = 0, fl = 0;
        for (u32 j0 = 0; j0 < s; j0 += 4) {               // (four records per turn of LDS reads, no branch: see bin_sort_index_kernel)
          u64 b0[4], b1[4], bm[4];
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const u32 jj = (j0 + (u32) i < s) ? j0 + (u32) i : s - 1u;
            b0[i] = R[3 * jj]; b1[i] = R[3 * jj + 1]; bm[i] = R[3 * jj + 2];
          }
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const u32 j = j0 + (u32) i;
            const bool live = j < s;                        // (uniform)
            const u64 bl = bm[i] & lmask;
            const bool same = live & (b0[i] == a0) & (b1[i] == a1) & (bl == al);
            const bool before = live & ((b0[i] > a0) | ((b0[i] == a0) & ((b1[i] > a1) | ((b1[i] == a1) & (bl > al)))));
            r += before ? 1u : 0u;
            rep = rep & !(same & (j < t));
            tot += same ? (u32) meta_count (bm[i]) : 0u;
            fl |= same ? (u32) (bm[i] >> TJ_META_FLAG_SHIFT) & 7u : 0u;
          }
        }
        H[t] = r | (rep ? 0x80000000u : 0u);
        // (the key's depth over all samples, 20-bit store, and the strands any sample saw it on)
        ttot[st + t] = rep ? ((tot & 0xFFFFFu) | (fl << 28)) : 0xFFFFFFFFu;
      }
      nrep += (u32) __popcll (__ballot (rep));
    }
    asm volatile ("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier ();
    for (u32 t = lane; t < s; t += 64) {                // pass 2: distinct keys in front = representatives with fewer records in front
      const u32 r = H[t] & 0x7FFFFFFFu;
      u32 d = 0;
      for (u32 j = 0; j < s; j += 4) {                    // (four entries per LDS read; entries past the bin's end hold an earlier bin's)
        const uint4 h = *reinterpret_cast<const uint4 *> (&H[j]);
        d += ((h.x & 0x80000000u) && (h.x & 0x7FFFFFFFu) < r) ? 1u : 0u;
        d += (j + 1u < s && (h.y & 0x80000000u) && (h.y & 0x7FFFFFFFu) < r) ? 1u : 0u;
        d += (j + 2u < s && (h.z & 0x80000000u) && (h.z & 0x7FFFFFFFu) < r) ? 1u : 0u;
        d += (j + 3u < s && (h.w & 0x80000000u) && (h.w & 0x7FFFFFFFu) < r) ? 1u : 0u;
      }
      tpos[st + t] = d;
    }
    if (lane == 0) binctx[bin] = nrep;
    asm volatile ("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier ();
  }
}

// union keys in order with the total depth in the count field, and the per-sample depth matrix
__global__ __launch_bounds__ (256)
void bin_merge_write_kernel (const u64 *__restrict__ rec, const u32 *__restrict__ binstart, const u32 *__restrict__ binout, int nbins, const FinCounts *fin,
                             const u32 *__restrict__ tpos, const u32 *__restrict__ ttot, int n_samples,
                             u64 *__restrict__ keys, int *__restrict__ counts, long cap)
{
  if (fin->sort_fallback) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int bin = blockIdx.x * 4 + wave; bin < nbins; bin += gridDim.x * 4) {
    const u32 st = binstart[bin], s = binstart[bin + 1] - st, o0 = binout[bin];
    for (u32 t0 = 0; t0 < s; t0 += 64) {                // representatives come first in a bin's index order: rows are
      const u32 t = t0 + lane;                          // zeroed (same wave, program order) before anybody fills them
      if (t < s) {
        const long u = (long) o0 + tpos[st + t];
        if (u < cap) {
          const u64 a0 = rec[3 * (u64) (st + t)], a1 = rec[3 * (u64) (st + t) + 1], am = rec[3 * (u64) (st + t) + 2];
          const u32 tot = ttot[st + t];
          if (tot != 0xFFFFFFFFu) {
            for (int q = 0; q < n_samples; q++) counts[u * n_samples + q] = 0;
            u64 m = am & ((1ull << TJ_META_SAMPLE_SHIFT) - 1ull);
            m = (m & ~(0xFFFFFull << TJ_META_COUNT_SHIFT)) | (((u64) tot & 0xFFFFFull) << TJ_META_COUNT_SHIFT);
            m = (m & ~(7ull << TJ_META_FLAG_SHIFT)) | ((u64) ((tot >> 28) & 7u) << TJ_META_FLAG_SHIFT);
            keys[3 * u] = a0; keys[3 * u + 1] = a1; keys[3 * u + 2] = m;
          }
        }
      }
      __builtin_amdgcn_wave_barrier ();
      asm volatile ("s_waitcnt vmcnt(0)" ::: "memory");
      if (t < s) {
        const long u = (long) o0 + tpos[st + t];
        if (u < cap) {
          const u64 am = rec[3 * (u64) (st + t) + 2];
          counts[u * n_samples + (int) (am >> TJ_META_SAMPLE_SHIFT)] = meta_count (am);
        }
      }
    }
  }
}

__global__ void set_int_kernel (int *p, int v) { *p = v; }

// ---- cross-sample merge, radix path (context-keyed union of the samples' histograms; reference precursor: src/genome_set.c:250-289)

__global__ void merge_tag_kernel (const u64 *__restrict__ in, u64 *__restrict__ out, long n, const long *__restrict__ starts, int n_samples)
{ // copy + write the sample index of every record into the spare bits of its meta word
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    int lo = 0, hi = n_samples;                         // starts[s] <= i < starts[s + 1]
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (starts[mid] <= i) lo = mid; else hi = mid; }
    out[3 * i] = in[3 * i]; out[3 * i + 1] = in[3 * i + 1];
    out[3 * i + 2] = (in[3 * i + 2] & ((1ull << TJ_META_SAMPLE_SHIFT) - 1ull)) | ((u64) lo << TJ_META_SAMPLE_SHIFT);
  }
}

__global__ void merge_write_kernel (const u64 *__restrict__ rec, long n, const u32 *__restrict__ flags, const u32 *__restrict__ segid,
                                    int n_samples, u64 *__restrict__ keys, int *__restrict__ counts, u32 *__restrict__ totals, u32 *__restrict__ orflags, long cap)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    const u32 seg = segid[i] + flags[i] - 1u;           // exclusive scan of the head flags: heads before i (+ itself) - 1
    if ((long) seg >= cap) continue;
    const u64 meta = rec[3 * i + 2];
    const int sample = (int) (meta >> TJ_META_SAMPLE_SHIFT);
    const int cnt = meta_count (meta);
    counts[(long) seg * n_samples + sample] = cnt;
    atomicAdd (&totals[seg], (u32) cnt);
    atomicOr (&orflags[seg], (u32) (meta >> TJ_META_FLAG_SHIFT) & 7u);
    if (flags[i]) { keys[3 * (long) seg] = rec[3 * i]; keys[3 * (long) seg + 1] = rec[3 * i + 1]; keys[3 * (long) seg + 2] = meta; }
  }
}

__global__ void merge_totals_kernel (u64 *__restrict__ keys, const u32 *__restrict__ totals, const u32 *__restrict__ orflags, const u32 *n_seg_p, long cap)
{ // count field := depth over all samples (20-bit store), canon_flag := the strands any sample saw the key on
  const long n_seg = min ((long) *n_seg_p, cap);
  for (long j = blockIdx.x * (long) blockDim.x + threadIdx.x; j < n_seg; j += (long) gridDim.x * blockDim.x) {
    u64 m = keys[3 * j + 2] & ((1ull << TJ_META_SAMPLE_SHIFT) - 1ull);
    m = (m & ~(0xFFFFFull << TJ_META_COUNT_SHIFT)) | (((u64) totals[j] & 0xFFFFFull) << TJ_META_COUNT_SHIFT);
    m = (m & ~(7ull << TJ_META_FLAG_SHIFT)) | ((u64) (orflags[j] & 7u) << TJ_META_FLAG_SHIFT);
    keys[3 * j + 2] = m;
  }
}


// ---------------------------------------------------------------------------------------------------------------
// host side of the thin layer

struct DevBuf
{
  void *p = nullptr;
  size_t cap = 0;
};

#define TJ_SCAN_PIECE_TARGET (1ull << 30)               // a long stream is scanned in pieces of 1 GiB; up to 1.5 GiB goes in one launch

// everything the host reads back: one device block, one pinned mirror
// (each part on cache lines of its own: the scan's workgroups hammer ctr and cursors with atomics)
// (snap_*: what ctr and cursors held when clear_buckets_kernel emptied them in a finalise -- the host reads the counts of
// the sample from there, with the one copy at the end of the finalise, instead of copying the block before the clear)
struct DevState { alignas (256) DevCounters ctr; alignas (256) FinCounts fin; alignas (256) u32 cursors[TJ_P + 1]; alignas (256) FinPlan plan;
                  alignas (256) DevCounters snap_ctr; alignas (256) u32 snap_cursors[TJ_P + 1]; alignas (256) u32 pad[4]; };

// One timed interval of a stream: an event in front of the stage's first kernel, one behind its last.  `timed` is the
// caller's to set: true once the stage has completed, false again where a call that may fail starts (a failed call leaves
// no timing behind); until then the interval reads as -1.
struct StageTimer
{
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool timed = false;
  hipError_t create () { const hipError_t e = hipEventCreate (&e0); return e != hipSuccess ? e : hipEventCreate (&e1); }
  void destroy () { if (e0) (void) hipEventDestroy (e0); if (e1) (void) hipEventDestroy (e1); }
  hipError_t begin (hipStream_t stream) { return hipEventRecord (e0, stream); }
  hipError_t end (hipStream_t stream) { return hipEventRecord (e1, stream); }
  bool elapsed (int device, float &ms) const           // waits for the end event
  { return timed && hipSetDevice (device) == hipSuccess && hipEventSynchronize (e1) == hipSuccess && hipEventElapsedTime (&ms, e0, e1) == hipSuccess; }
  double ms (int device) const { float f = 0.f; return elapsed (device, f) ? (double) f : -1.0; }
};
// the intervals of a counter: the last scan call (its partition kernels between the pieces included: tjamd_last_scan_ms takes
// them out), finalise, the kernels of tjamd_merge_samples, tjamd_tract_stats, tjamd_union_tracts, tjamd_union_tract_stats
enum { T_SCAN, T_FIN, T_MERGE, T_TRACT, T_UNION, T_UNION_STATS, T_REF, T_LOCATE, T_LOCATED_TRACTS, T_VARIANTS, T_ANNOTATION, T_TRACT_FEATURES, T_SEED_ORDER, T_LOCATE_GAPPED, T_CODING, T_VARIANT_EFFECTS, T_MERGE_VARIANTS, T_SITE_DEPTHS, T_SAMPLE_DISTANCES, T_SAMPLE_LINKAGE, T_LINKAGE_CLUSTERS, T_GROUP_SITES, T_LINKAGE_TREE, T_CLADE_SITES, T_SAMPLE_AGGLOMERATE, T_BOOTSTRAP_WEIGHTS, T_SAMPLE_DISTANCES_WEIGHTED, T_CLADE_SUPPORT, T_REPLICATE_TREES, T_CONSENSUS_TREE, TJ_N_TIMERS };   // (T_REF to T_LOCATED_TRACTS: N7, T_VARIANTS: N8, the next two: N9; then two of N10; two of N11; then N12, N13, N14, the two of N15, N16, the two of N17, N18, the three of N19, N20 and N21, end of the file)

// A finalise between its two halves: finalise_queue fills this in, finalise_collect reads it and sets the state back to
// FIN_IDLE (nothing begun).  FIN_EVENT: begun, ev_done says when the counts have arrived; FIN_ARRIVED: begun, the stream has
// been waited for and nothing is left to wait for; FIN_SETTLED: the outcome was clear at once (no raw records), c->status has it.
enum FinState { FIN_IDLE, FIN_EVENT, FIN_ARRIVED, FIN_SETTLED };
struct FinCarry { FinState state = FIN_IDLE; int remove_biased = 0, min_coverage = 0; bool speculative = false, plan_ahead = false; u64 kept_cap = 0; };

struct tjamd_counter
{
  int device = 0, k = 0, W = 4, n_cu = 256;
  hipStream_t own_stream = nullptr, stream = nullptr;
  DevCounters *d_ctr = nullptr, *h_ctr = nullptr;     // scan counters (device / pinned host mirror)
  DevCounters *d_lctr = nullptr;                      // located-list counters
  u32 *d_cursors = nullptr, *h_cursors = nullptr;     // [TJ_P] records per bucket, then [TJ_P] = next free chunk
  DevBuf pool, table, stage, fix, loc, prefix, rawlist, slow;
  DevBuf log, logmeta;        // the record log of scan_fast_kernel<1, true> and its block counters (2 words: blocks handed out, by launch parity; then a count per block)
  int log_mode = 1;           // widest record (words) that goes through the record log and partition_log_kernel: 1 = k <= 12 (default), 2 = k <= 28 as well
                              // (TATAJUBA_AMD_SINK=log), 0 = none, the scan kernels partition by themselves (TATAJUBA_AMD_SINK=fused)
  bool log_next_clean[2] = {false, false};
  hipEvent_t ev_p1 = nullptr; // after the partition kernel of the last scan call
  // a stream scanned in pieces runs scan, partition, scan, partition, ...: an event in front of every partition kernel but the
  // last and one behind it, so that the scan's and the partition's times can be told apart (TJ_PIECE_EVENTS pieces; beyond: lumped)
#define TJ_PIECE_EVENTS 64
  hipEvent_t ev_pa[TJ_PIECE_EVENTS] = {}, ev_pb[TJ_PIECE_EVENTS] = {};
  int n_piece_ev = 0;
  StageTimer timer[TJ_N_TIMERS];
  DevBuf ts_cov, ts_aux;      // tjamd_tract_stats / tjamd_tract_sample_stats: the samples' coverages, error flag + last tract id
  long union_cand = -1;       // retry candidates of the last tjamd_union_tracts
  DevBuf ut_tot, ut_lev, ut_fb, ut_slots;   // union tracts: exact row totals, admitted edit distances, fallback flags, global bars
  DevBuf lc_work;             // N7 (reference index, locate, located tracts): one block of scratch, cut up per call
  bool part_timed = false;    // the last scan call went through partition_log_kernel: timer[T_SCAN].e1 to ev_p1 is its time
  int fast_mode = 1;          // 1: scan_fast_kernel + the generic kernel on what it leaves; 0: generic kernel only; 2: fast kernel leaves everything (tests)
  u32 pool_chunks = 0, maxj = 0;
  int ch_shift = -1;          // chunk = TJ_CH0 << ch_shift records; fixed by the first scan after a reset
  u64 bucket_bound = 0;       // upper bound of the fullest bucket (exact after a synchronisation)
  u64 chunk_bound = 0;        // upper bound of the chunks handed out
  long n_raw_known = 0;       // exact after the last synchronisation
  u64 raw_bound = 0;          // upper bound of the raw records in the buckets (exact after a synchronisation)
  long n_undefined = 0;
  double slack = 1.0;
  DevBuf alt, hist, flags, segid, headpos, keep, outpos, scan_tmp, kept, idx_i, idx_f, cov, bins, binstart, binctx, ovf, grp_jt, grp_hist, fine;
  u32 bin_rank_max = BS_RANK_MAX;
  FinCounts *d_fin = nullptr, *h_fin = nullptr;
  struct DevState *d_state = nullptr, *h_state = nullptr;   // ctr, fin and cursors live in one block: one copy brings all three to the host
  void *h_kept = nullptr; size_t h_kept_cap = 0;   // pinned landing place of tjamd_download_kept (grown, never per call)
  bool bins_zeroed = false;
  bool fine_dirty = false;              // the fine bins hold an aggregation's counts that no clear_buckets_kernel has consumed yet
  bool bins_counted = false;            // clear_buckets_kernel has turned them into the ordering step's bin counts (finalise_binned: no counting pass)
  long n_kept = 0; int n_idx = 0, coverage = 0, status = -1;
  hipEvent_t ev_done = nullptr;                         // tjamd_finalise_begin: the counts have reached the host
  hipEvent_t ev_agg = nullptr;                          // the aggregation and the clearing of the buckets are done (order_stream waits for it)
  hipStream_t order_stream = nullptr;                   // tjamd_counter_set_order_stream: where a finalise begun with tjamd_finalise_begin runs its ordering step
  // where that step goes: ORDER_SIDE (default) the library's own side stream of the device, taken when first needed
  // (side_stream_acquire); ORDER_MAIN (TATAJUBA_AMD_ORDER=main) the counter's stream; ORDER_GIVEN what
  // tjamd_counter_set_order_stream said, a stream or none
  enum { ORDER_SIDE, ORDER_MAIN, ORDER_GIVEN } order_mode = ORDER_SIDE;
  bool side_held = false;                               // this counter counts among the users of its device's side stream
  unsigned order_path = 0;                              // tjamd_debug_order_path: how the last finalise ran its ordering step
  FinCarry fin;                                         // what finalise_queue leaves for finalise_collect
  hipEvent_t marks[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // tjamd_mark / tjamd_wait_mark
  unsigned mark_seq = 0;
  long last_scan_launches = 0;
  unsigned scan_seq = 0;
  size_t piece_target = TJ_SCAN_PIECE_TARGET;           // TATAJUBA_AMD_SCAN_PIECE (bytes) overrides it: tests
  int scan_grid_cap = 0;                                // TATAJUBA_AMD_SCAN_GRID (tests): n >= 1 caps the workgroups of the scan and log-partition launches; 0: no cap
  int dist_blocks = 0;                                  // TATAJUBA_AMD_DISTANCE_BLOCKS (tests): the workgroups tjamd_sample_distances and tjamd_sample_distances_weighted split their sites for; 0: four per CU
  int link_small = 1;                                   // TATAJUBA_AMD_LINKAGE_SMALL (tests): 0: tjamd_sample_linkage never takes its single-workgroup path (64 samples and fewer)
  int aggl_batch = 32;                                  // TATAJUBA_AMD_AGGL_BATCH (tools, tests): the rounds tjamd_sample_agglomerate enqueues between two looks at its flag words; AGGL_BATCH
  int trees_group = 0;                                  // TATAJUBA_AMD_TREES_GROUP (tests, tools): n >= 1: the replicates tjamd_replicate_trees takes through at a time; 0: what 1 GiB of scratch holds
  int consensus_key_bits = 51;                          // TATAJUBA_AMD_CONSENSUS_KEY_BITS (tests): b in 0 .. 51: the bits of the hash sum that tjamd_consensus_tree keeps in a clade's key; CONS_KEY_BITS
  int groups_small = 1;                                 // TATAJUBA_AMD_GROUPS_SMALL (tests): 0: tjamd_group_sites never takes its wavefront-per-site form (64 samples and fewer)
  int clades_small = 1;                                 // TATAJUBA_AMD_CLADES_SMALL (tests): 0: tjamd_clade_sites never takes its wavefront-per-site form (64 samples and fewer)
  int fastq_carry_max = TJAMD_FASTQ_CARRY_MAX;         // TATAJUBA_AMD_FASTQ_CARRY (tests): n >= 16 bytes: the longest record a push boundary of a tjamd_fastq_* session may cut
  struct FastqSession *fq = nullptr;                    // tjamd_fastq_*: made by the first tjamd_fastq_begin (end of the file)
  bool buckets_clean = false;
  long plan_mismatches = 0;   // finalises whose in-kernel reading of the kept count differed from the kernel boundary's (expected: 0)
  bool ctr_clean = false;     // the scan counters are zero but for n_undefined (clear_buckets_kernel did it, no scan since)
};

static int ensure (DevBuf &b, size_t bytes, hipStream_t stream, size_t keep_bytes = 0)
{
  if (bytes <= b.cap) return TJAMD_OK;
  size_t want = std::max (bytes, b.cap + b.cap / 2);
  void *np = nullptr;
  hipError_t e = hipMalloc (&np, want);
  if (e != hipSuccess && want > bytes) { want = bytes; e = hipMalloc (&np, want); }
  if (e != hipSuccess) return set_err (TJAMD_ERR_HIP, "hipMalloc of %zu bytes failed: %s", want, hipGetErrorString (e));
  if (b.p) {
    if (keep_bytes) HIPCHK (hipMemcpyAsync (np, b.p, keep_bytes, hipMemcpyDeviceToDevice, stream));
    HIPCHK (hipStreamSynchronize (stream));
    HIPCHK (hipFree (b.p));
  }
  b.p = np; b.cap = want;
  return TJAMD_OK;
}

static void release (DevBuf &b) { if (b.p) (void) hipFree (b.p); b.p = nullptr; b.cap = 0; }

// The record width of a counter (c->W: 1, 2 or 4 words) as a compile-time constant: f is called with
// std::integral_constant<int, W>, so that `constexpr int W = decltype (w)::value` names the kernel instance to launch.
template <class F> static void with_width (int W, F &&f)
{
  switch (W) {
    case 1: f (std::integral_constant<int, 1> ()); break;
    case 2: f (std::integral_constant<int, 2> ()); break;
    default: f (std::integral_constant<int, 4> ()); break;
  }
}

// the T_FIN interval ends here on this stream, and counts
static int end_fin_interval (tjamd_counter *c, hipStream_t stream) { HIPCHK (c->timer[T_FIN].end (stream)); c->timer[T_FIN].timed = true; return TJAMD_OK; }
// this finalise is over with status s: in the counter, and through the caller's pointer where there is one
static int finalise_status (tjamd_counter *c, int *status, int s) { c->status = s; if (status) *status = s; return TJAMD_OK; }

// One call's use of a timer of its counter.  Construction clears `timed` (where the entry does that relative to its checks is
// the entry's choice; a null counter, or one that stands for a counter where there is no device, is left alone), begin ()
// and end () record on the counter's stream, done () marks the interval as good.  A call that leaves by any other way has
// no timing: "a failed call leaves no timing behind" holds without the author's care.  enter () is the head of a device call whose
// argument checks are done: the refusal without a device (`what`: the clause that says what the device does), then the counter's device.
struct Stage
{
  tjamd_counter *c; StageTimer *t;
  Stage (tjamd_counter *c_, int slot) : c (c_), t (c_ && tjamd_device_count () > 0 ? &c_->timer[slot] : nullptr) { if (t) t->timed = false; }
  int enter (const char *fn, const char *what)
  { // 0, or the code of the step that fails with its message set
    if (tjamd_device_count () <= 0) return set_err (TJAMD_ERR_NO_DEVICE, "%s: TJAMD_ERR_NO_DEVICE: no HIP device visible (%s on the device; no CPU fallback)", fn, what);
    return hipSetDevice (c->device) == hipSuccess ? TJAMD_OK : set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  }
  void begin () { (void) t->begin (c->stream); }
  void end () { (void) t->end (c->stream); }
  void done () { t->timed = true; }
};
// the getter of a slot's last interval: milliseconds, -1.0 for a null counter or where the last call left no timing
#define TJ_LAST_MS(name, slot) extern "C" double name (tjamd_counter *c) { return c ? c->timer[slot].ms (c->device) : -1.0; }

// The scratch of one call, cut from c->lc_work: each piece is listed once, in the order it lies in the block, on a 256-byte
// boundary.  take () only notes the caller's pointer and the piece's offset; commit () grows the block once (which may
// free and replace it) and then hands every piece out.  Until then the pointers hold nothing.
struct ScratchCut
{
  struct Piece { void *at; size_t offset; void (*put) (void *at, char *p); } piece[16];
  int n = 0; size_t used = 0;
  template <class T> void take (T *&p, size_t count)
  {
    p = nullptr;
    if (n < 16) piece[n] = Piece {&p, used, [] (void *at, char *q) { *(T **) at = (T *) q; }};
    n++; used += (count * sizeof (T) + 255) & ~(size_t) 255;
  }
  int commit (tjamd_counter *c)
  {
    if (n > 16) return set_err (TJAMD_ERR_STATE, "a scratch cut of %d pieces (16 at most)", n);
    const int rc = ensure (c->lc_work, used, c->stream);
    for (int i = 0; i < n && !rc; i++) piece[i].put (piece[i].at, (char *) c->lc_work.p + piece[i].offset);
    return rc;
  }
};

// The 64 flag words of a call (ints, or the type of the call's count) as the last piece of its cut: takes them, commits the cut and
// clears them on the counter's stream.  flags_alone: the same for a call with no other scratch, the words at the head of c->lc_work.
template <class T> static int commit_with_flags (ScratchCut &cut, tjamd_counter *c, const char *fn, T *&flags)
{
  static_assert (sizeof (T) == 4, "a flag word");
  cut.take (flags, 64);
  const int rc = cut.commit (c);
  if (rc) return rc;
  return hipMemsetAsync (flags, 0, 256, c->stream) == hipSuccess ? TJAMD_OK : set_err (TJAMD_ERR_HIP, "%s: memset failed", fn);
}
template <class T> static int flags_alone (tjamd_counter *c, const char *fn, T *&flags) { ScratchCut cut; return commit_with_flags (cut, c, fn, flags); }

// The tail of a call, behind its stage's end (): the error of its launches, the copy of `words` 32-bit words from d to the
// host (none: the wait alone) on the counter's stream, the wait for the stream.  Decoding the words is the caller's.
static int read_back (tjamd_counter *c, const char *fn, const void *d, void *h, size_t words)
{
  hipError_t e = hipGetLastError ();
  if (e == hipSuccess && words) e = hipMemcpyAsync (h, d, words * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize (c->stream);
  return e == hipSuccess ? TJAMD_OK : set_err (TJAMD_ERR_HIP, "%s: failed: %s", fn, hipGetErrorString (e));
}

// The library's side stream: one per device for the whole process, where the ordering step of a begun finalise runs
// beside the next sample's scan.  Made when a counter first needs it, shared by every counter of the device (their
// steps follow each other on it, as they did on one stream), destroyed with the last counter that used it.  Not one per
// counter: a process has few hardware queues, and streams that share a queue run one after the other.
#define TJ_SIDE_DEVICES 64
static std::mutex g_side_mutex;
static struct { hipStream_t stream; int users; } g_side[TJ_SIDE_DEVICES];

static hipStream_t side_stream_acquire (tjamd_counter *c)
{ // null: no such stream (the step then stays on the counter's stream)
  if (c->device < 0 || c->device >= TJ_SIDE_DEVICES) return nullptr;
  std::lock_guard<std::mutex> lock (g_side_mutex);
  auto &s = g_side[c->device];
  if (!c->side_held) {
    if (!s.stream && hipStreamCreateWithFlags (&s.stream, hipStreamNonBlocking) != hipSuccess) { s.stream = nullptr; (void) hipGetLastError (); return nullptr; }
    s.users++; c->side_held = true;
  }
  return s.stream;
}

static void side_stream_release (tjamd_counter *c)
{
  if (!c->side_held) return;
  std::lock_guard<std::mutex> lock (g_side_mutex);
  auto &s = g_side[c->device];
  c->side_held = false;
  if (--s.users == 0 && s.stream) { (void) hipStreamSynchronize (s.stream); (void) hipStreamDestroy (s.stream); s.stream = nullptr; }
}

extern "C" tjamd_counter *tjamd_counter_create (int device, int kmer_size)
{
  int n = tjamd_device_count ();
  if (n <= 0) { set_err (TJAMD_ERR_NO_DEVICE, "no HIP device visible: the homopolymer-tract engine needs an MI355X (no CPU fallback)"); return NULL; }
  if (device < 0 || device >= n) { set_err (TJAMD_ERR_ARG, "device %d out of range [0,%d)", device, n); return NULL; }
  if (kmer_size < 2 || kmer_size > 32) { set_err (TJAMD_ERR_ARG, "kmer_size %d outside [2,32] (reference clamp: src/main.c:184-185)", kmer_size); return NULL; }
  HIPCHK_NULL (hipSetDevice (device));
  // (a failure below leaves through tjamd_counter_destroy, which takes a counter built this far)
  std::unique_ptr<tjamd_counter, void (*) (tjamd_counter *)> made (new tjamd_counter (), tjamd_counter_destroy);
  tjamd_counter *const c = made.get ();
  c->device = device; c->k = kmer_size;
  c->W = (kmer_size <= 12) ? 1 : (kmer_size <= 28) ? 2 : 4;
  hipDeviceProp_t prop;
  HIPCHK_NULL (hipGetDeviceProperties (&prop, device));
  c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  const char *bm = getenv ("TATAJUBA_AMD_BIN_MAX");      // test hook: a smaller limit forces the radix path
  if (bm && atoi (bm) >= 1 && atoi (bm) <= BS_RANK_MAX) c->bin_rank_max = (u32) atoi (bm);
  const char *pc = getenv ("TATAJUBA_AMD_SCAN_PIECE");
  if (pc && atol (pc) >= 4096) c->piece_target = (size_t) atol (pc);
  const char *sk = getenv ("TATAJUBA_AMD_SINK");          // "fused": scan_fast_kernel<1> partitions its records itself (rounds 1-3); default: record log + partition_log_kernel
  if (sk && !strcmp (sk, "fused")) c->log_mode = 0;
  if (sk && !strcmp (sk, "log")) c->log_mode = 2;
  const char *om = getenv ("TATAJUBA_AMD_ORDER");         // "main": the ordering step of a begun finalise stays on the counter's stream (no side stream); read here, kept in the counter
  if (om && !strcmp (om, "main")) c->order_mode = tjamd_counter::ORDER_MAIN;
  const char *fm = getenv ("TATAJUBA_AMD_FAST");          // test hook: 0 = generic scan kernel only, 2 = fast kernel hands every tile over
  if (fm && atoi (fm) >= 0 && atoi (fm) <= 2) c->fast_mode = atoi (fm);
  const char *sg = getenv ("TATAJUBA_AMD_SCAN_GRID");     // test hook: at most n workgroups per scan / log-partition launch (one workgroup then walks many tiles or blocks)
  if (sg && atoi (sg) >= 1) c->scan_grid_cap = atoi (sg);
  const char *db = getenv ("TATAJUBA_AMD_DISTANCE_BLOCKS");   // test hook: tjamd_sample_distances aims at n workgroups when it splits the sites (1: never splits)
  if (db && atoi (db) >= 1) c->dist_blocks = atoi (db);
  const char *ls = getenv ("TATAJUBA_AMD_LINKAGE_SMALL");    // test hook: 0 sends every tjamd_sample_linkage through the key pass, the rounds and the sort kernel
  if (ls && !strcmp (ls, "0")) c->link_small = 0;
  const char *ab = getenv ("TATAJUBA_AMD_AGGL_BATCH");       // measuring hook: n >= 1 rounds of tjamd_sample_agglomerate per look at the flag words
  if (ab && atoi (ab) >= 1) c->aggl_batch = atoi (ab);
  const char *tg = getenv ("TATAJUBA_AMD_TREES_GROUP");      // test hook: n >= 1 replicates of tjamd_replicate_trees per group
  if (tg && atoi (tg) >= 1) c->trees_group = atoi (tg);
  const char *kb = getenv ("TATAJUBA_AMD_CONSENSUS_KEY_BITS");   // test hook: fewer bits put different clades into one run of tjamd_consensus_tree, which then tells them apart by comparison
  if (kb && *kb && atoi (kb) >= 0) c->consensus_key_bits = std::min (atoi (kb), 51);
  const char *gs = getenv ("TATAJUBA_AMD_GROUPS_SMALL");     // test hook: 0 sends every tjamd_group_sites through the workgroup-per-run form with its LDS tables
  if (gs && !strcmp (gs, "0")) c->groups_small = 0;
  const char *cs = getenv ("TATAJUBA_AMD_CLADES_SMALL");     // test hook: 0 sends every tjamd_clade_sites through the workgroup-per-run form with its LDS scans
  if (cs && !strcmp (cs, "0")) c->clades_small = 0;
  const char *fc = getenv ("TATAJUBA_AMD_FASTQ_CARRY");     // test hook: a shorter carry for the tjamd_fastq_* sessions of this counter
  if (fc && atoi (fc) >= 16 && atoi (fc) <= TJAMD_FASTQ_CARRY_MAX) c->fastq_carry_max = atoi (fc);
  const char *sl = getenv ("TATAJUBA_AMD_BUCKET_SLACK");
  if (sl && atof (sl) >= 1.0) c->slack = atof (sl);
  HIPCHK_NULL (hipStreamCreateWithFlags (&c->own_stream, hipStreamNonBlocking));
  c->stream = c->own_stream;
  HIPCHK_NULL (hipMalloc ((void **) &c->d_state, sizeof (DevState)));
  HIPCHK_NULL (hipMalloc ((void **) &c->d_lctr, sizeof (DevCounters)));
  HIPCHK_NULL (hipHostMalloc ((void **) &c->h_state, sizeof (DevState), hipHostMallocDefault));
  c->d_ctr = &c->d_state->ctr; c->d_fin = &c->d_state->fin;
  HIPCHK_NULL (hipMalloc ((void **) &c->d_cursors, (size_t) (TJ_P + 1) * TJ_CSTRIDE * 4));     // (strided: see TJ_CSTRIDE; d_state->cursors is the packed copy the host reads)
  HIPCHK_NULL (hipMemsetAsync (c->d_cursors, 0, (size_t) (TJ_P + 1) * TJ_CSTRIDE * 4, c->stream));
  c->h_ctr = &c->h_state->ctr; c->h_fin = &c->h_state->fin; c->h_cursors = c->h_state->cursors;
  memset (c->h_state, 0, sizeof (DevState));
  HIPCHK_NULL (hipMemsetAsync (c->d_state, 0, sizeof (DevState), c->stream));
  HIPCHK_NULL (hipMemsetAsync (c->d_lctr, 0, sizeof (DevCounters), c->stream));
  for (StageTimer &t : c->timer) HIPCHK_NULL (t.create ());
  HIPCHK_NULL (hipEventCreate (&c->ev_p1));
  HIPCHK_NULL (hipEventCreateWithFlags (&c->ev_done, hipEventDisableTiming));
  HIPCHK_NULL (hipEventCreateWithFlags (&c->ev_agg, hipEventDisableTiming));
  HIPCHK_NULL (hipStreamSynchronize (c->stream));
  return made.release ();
}

static void fastq_release (tjamd_counter *c);         // (the buffers, events and pinned memory of its tjamd_fastq_* sessions)

extern "C" void tjamd_counter_destroy (tjamd_counter *c)
{
  if (!c) return;
  (void) hipSetDevice (c->device);
  if (c->stream) (void) hipStreamSynchronize (c->stream);   // (null: tjamd_counter_create got no further than that)
  if (c->fin.state == FIN_EVENT) (void) hipEventSynchronize (c->ev_done);   // (begun and never ended: its ordering step may be on another stream)
  side_stream_release (c);
  fastq_release (c);
  DevBuf *all[] = {&c->log, &c->logmeta, &c->pool, &c->table, &c->stage, &c->fix, &c->loc, &c->prefix, &c->rawlist, &c->slow, &c->alt, &c->hist, &c->flags, &c->segid, &c->headpos,
                   &c->keep, &c->outpos, &c->scan_tmp, &c->kept, &c->idx_i, &c->idx_f, &c->cov, &c->bins, &c->binstart, &c->binctx, &c->ovf, &c->grp_jt, &c->grp_hist, &c->fine,
                   &c->ts_cov, &c->ts_aux, &c->ut_tot, &c->ut_lev, &c->ut_fb, &c->ut_slots, &c->lc_work};
  for (DevBuf *b : all) release (*b);
  for (hipEvent_t ev : c->marks) if (ev) (void) hipEventDestroy (ev);
  if (c->d_state) (void) hipFree (c->d_state);
  if (c->d_lctr) (void) hipFree (c->d_lctr);
  if (c->d_cursors) (void) hipFree (c->d_cursors);
  if (c->h_state) (void) hipHostFree (c->h_state);
  if (c->h_kept) (void) hipHostFree (c->h_kept);
  for (StageTimer &t : c->timer) t.destroy ();
  if (c->ev_p1) (void) hipEventDestroy (c->ev_p1);
  for (int i = 0; i < TJ_PIECE_EVENTS; i++) { if (c->ev_pa[i]) (void) hipEventDestroy (c->ev_pa[i]); if (c->ev_pb[i]) (void) hipEventDestroy (c->ev_pb[i]); }
  if (c->ev_done) (void) hipEventDestroy (c->ev_done);
  if (c->ev_agg) (void) hipEventDestroy (c->ev_agg);
  if (c->own_stream) (void) hipStreamDestroy (c->own_stream);
  delete c;
}

extern "C" int tjamd_counter_device (const tjamd_counter *c) { return c ? c->device : -1; }

extern "C" int tjamd_counter_set_stream (tjamd_counter *c, void *hip_stream)
{
  if (!c) return set_err (TJAMD_ERR_ARG, "null counter");
  HIPCHK (hipSetDevice (c->device));
  HIPCHK (hipStreamSynchronize (c->stream));
  // A counter on a caller's stream holds no stream of its own: a process has few hardware queues (four by default),
  // streams that share one run one after the other, and the side stream of the ordering step must not land on the
  // queue of the stream it is to run beside -- with two idle own streams on two of the queues it did, in every step of
  // the bench (profiles/README.md, "Ordering step beside the next scan").
  if (hip_stream) {
    if (c->own_stream) { HIPCHK (hipStreamDestroy (c->own_stream)); c->own_stream = nullptr; }
    c->stream = (hipStream_t) hip_stream;
  }
  else {
    if (!c->own_stream) HIPCHK (hipStreamCreateWithFlags (&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
  }
  return TJAMD_OK;
}

// The stream for the ordering step of a finalise that was begun with tjamd_finalise_begin, named by the caller (null:
// none, the step stays on the counter's stream).  The step is six small launches whose time is latency, not work (76 us
// for 235 k records), each sized to start on a CU that three workgroups of scan_fast_kernel<1, true> fill (ORDER_KERNEL):
// behind an event on the counter's stream it runs beside whatever that stream does next -- the scan of the next sample
// on another counter -- and tjamd_finalise_end waits for its last copy as before.  The counter itself must not be
// touched between the two calls.  A counter on which this was never called uses the library's side stream
// (side_stream_acquire) unless TATAJUBA_AMD_ORDER=main was set when it was made.
extern "C" int tjamd_counter_set_order_stream (tjamd_counter *c, void *hip_stream)
{
  if (!c) return set_err (TJAMD_ERR_ARG, "null counter");
  HIPCHK (hipSetDevice (c->device));
  HIPCHK (hipStreamSynchronize (c->stream));
  if (c->fin.state == FIN_EVENT) HIPCHK (hipEventSynchronize (c->ev_done));   // (a step begun on the stream that is given up here)
  c->order_stream = (hipStream_t) hip_stream;
  c->order_mode = tjamd_counter::ORDER_GIVEN;
  return TJAMD_OK;
}

// diagnostic (tests): how the last finalise ran its ordering step, a sum of 1: planned ahead and queued on another stream than
// the counter's; 2: with the kept count in hand, on the counter's stream (nothing planned, or more kept than planned
// for); 4: planned ahead and queued on the counter's stream.  0: no ordering step (or no finalise).
extern "C" long tjamd_debug_order_path (tjamd_counter *c) { return c ? (long) c->order_path : -1; }

static Buckets make_buckets (const tjamd_counter *c)
{
  Buckets B;
  B.pool = (u64 *) c->pool.p; B.table = (u32 *) c->table.p; B.cursors = c->d_cursors; B.pool_next = c->d_cursors + TJ_P * TJ_CSTRIDE;
  B.pool_chunks = c->pool_chunks; B.maxj = c->maxj; B.ch_shift = (u32) std::max (c->ch_shift, 0);
  return B;
}

// forget every raw record: cursors and chunk counter to zero, chunk table to "unclaimed"
static int clear_buckets (tjamd_counter *c, bool snapshot = false)
{
  if (!c->buckets_clean || snapshot) {
    // (behind an aggregation that counted its kept records into the fine bins: this kernel turns them into the ordering
    // step's bin counts, see there)
    const bool fused = snapshot && c->fine_dirty && c->bins.p != nullptr;
    hipLaunchKernelGGL (clear_buckets_kernel, dim3 (TJ_P), dim3 (256), 0, c->stream, c->d_cursors, c->d_ctr,
                        (u32 *) (c->maxj ? c->table.p : nullptr), c->maxj, c->ch_shift, c->d_fin, (u32 *) c->bins.p, c->bins.p ? BS_MAXBINS : 0,
                        snapshot ? &c->d_state->snap_ctr : (DevCounters *) nullptr, snapshot ? c->d_state->snap_cursors : (u32 *) nullptr,
                        snapshot ? &c->d_state->plan : (FinPlan *) nullptr, fused ? (u32 *) c->fine.p : (u32 *) nullptr, fine_bin_bits (c->k));
    HIPCHK (hipGetLastError ());
    c->buckets_clean = true;
    c->ctr_clean = true;
    c->bins_zeroed = c->bins.p != nullptr && !fused;
    if (fused) { c->fine_dirty = false; c->bins_counted = true; }   // (the fine bins are zeroed again, the step's bins hold its counts if the plan is usable)
  }
  c->n_raw_known = 0; c->raw_bound = 0; c->bucket_bound = 0; c->chunk_bound = TJ_P; c->ch_shift = -1;
  return TJAMD_OK;
}

extern "C" int tjamd_counter_reset (tjamd_counter *c)
{
  if (!c) return set_err (TJAMD_ERR_ARG, "null counter");
  HIPCHK (hipSetDevice (c->device));
  // (the memset is not needed right after a finalise whose counts the host has seen: clear_buckets_kernel zeroed the rest)
  if (!(c->ctr_clean && c->fin.state == FIN_IDLE && c->n_undefined == 0)) HIPCHK (hipMemsetAsync (c->d_ctr, 0, sizeof (DevCounters), c->stream));
  int rc = clear_buckets (c);
  c->ctr_clean = true;
  if (rc) return rc;
  c->n_undefined = 0;
  c->n_kept = 0; c->n_idx = 0; c->coverage = 0; c->status = -1;
  return TJAMD_OK;
}

extern "C" void *tjamd_host_alloc (size_t bytes)
{
  void *p = nullptr;
  if (hipHostMalloc (&p, bytes, hipHostMallocPortable) != hipSuccess) { set_err (TJAMD_ERR_HIP, "hipHostMalloc of %zu bytes failed", bytes); return NULL; }   // (portable: batch buffers are pooled across the counters of all devices)
  return p;
}

extern "C" void tjamd_host_free (void *p) { if (p) (void) hipHostFree (p); }

// device memory for callers that have no HIP headers of their own (outputs of tjamd_merge_samples and the like)
extern "C" void *tjamd_device_alloc (tjamd_counter *c, size_t bytes)
{
  void *p = nullptr;
  if (!c || hipSetDevice (c->device) != hipSuccess || hipMalloc (&p, bytes ? bytes : 1) != hipSuccess) { set_err (TJAMD_ERR_HIP, "hipMalloc of %zu bytes failed", bytes); return NULL; }
  return p;
}
extern "C" void tjamd_device_free (tjamd_counter *c, void *p) { if (c && p && hipSetDevice (c->device) == hipSuccess) (void) hipFree (p); }
extern "C" int tjamd_device_download (tjamd_counter *c, void *host, const void *dev, size_t bytes)
{
  if (!c || (bytes && (!host || !dev))) return set_err (TJAMD_ERR_ARG, "bad arguments");
  HIPCHK (hipSetDevice (c->device));
  HIPCHK (hipStreamSynchronize (c->stream));
  if (bytes) HIPCHK (hipMemcpy (host, dev, bytes, hipMemcpyDeviceToHost));
  return TJAMD_OK;
}

extern "C" int tjamd_sync (tjamd_counter *c)
{
  if (!c) return set_err (TJAMD_ERR_ARG, "null counter");
  HIPCHK (hipSetDevice (c->device));
  HIPCHK (hipStreamSynchronize (c->stream));
  return TJAMD_OK;
}

// A mark is a point in the counter's stream (everything queued before it); waiting for a mark does not wait for what was
// queued after it.  The feeder uses marks to re-use a pinned batch buffer as soon as ITS copy and scan are done while
// later batches are still in flight.  Eight marks are live at a time (the ninth re-uses the first one's slot).
extern "C" int tjamd_mark (tjamd_counter *c)
{
  if (!c) return -set_err (TJAMD_ERR_ARG, "null counter");
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  const int slot = (int) (c->mark_seq++ & 7u);
  if (!c->marks[slot] && hipEventCreateWithFlags (&c->marks[slot], hipEventDisableTiming) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipEventCreate failed");
  if (hipEventRecord (c->marks[slot], c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipEventRecord failed");
  return slot;
}

extern "C" int tjamd_wait_mark (tjamd_counter *c, int mark)
{
  if (!c || mark < 0 || mark > 7 || !c->marks[mark]) return set_err (TJAMD_ERR_ARG, "bad mark");
  HIPCHK (hipSetDevice (c->device));
  HIPCHK (hipEventSynchronize (c->marks[mark]));
  return TJAMD_OK;
}

// stream synchronisation + exact counts
__global__ void pack_cursors_kernel (const u32 *__restrict__ cursors, u32 *__restrict__ packed)
{
  if (threadIdx.x <= TJ_P) packed[threadIdx.x] = cursors[threadIdx.x * TJ_CSTRIDE];
}

static int queue_counter_copies (tjamd_counter *c)
{
  hipLaunchKernelGGL (pack_cursors_kernel, dim3 (1), dim3 (320), 0, c->stream, (const u32 *) c->d_cursors, c->d_state->cursors);
  HIPCHK (hipGetLastError ());
  HIPCHK (hipMemcpyAsync (c->h_state, c->d_state, sizeof (DevState), hipMemcpyDeviceToHost, c->stream));
  return TJAMD_OK;
}

// the copies queued by queue_counter_copies() have arrived: errors, exact counts
static int apply_counter_copies (tjamd_counter *c, bool from_snapshot = false)
{
  long total = 0;
  u64 mx = 0;
  struct View { const DevCounters *h_ctr; const u32 *h_cursors; } v = {c->h_ctr, c->h_cursors};
  if (from_snapshot) { v.h_ctr = &c->h_state->snap_ctr; v.h_cursors = c->h_state->snap_cursors; }
  for (int b = 0; b < TJ_P; b++) { total += v.h_cursors[b]; mx = std::max<u64> (mx, v.h_cursors[b]); }
  if (v.h_ctr->overflow == 2u)
    return set_err (TJAMD_ERR_HIP, "a chunk of raw record storage was claimed but its id was never published (waited %u polls): "
                    "the claiming workgroup did not make progress -- please report; scanning again usually succeeds", (unsigned) TJ_SPIN_MAX);
  if (v.h_ctr->overflow)
    return set_err (TJAMD_ERR_CAPACITY, "raw record storage exhausted (%u of %u chunks handed out, fullest bucket %llu records): "
                    "raise TATAJUBA_AMD_BUCKET_SLACK (now %.1f) and scan again", v.h_cursors[TJ_P], c->pool_chunks, (unsigned long long) mx, c->slack);
  if (v.h_ctr->fix_overflow) return set_err (TJAMD_ERR_CAPACITY, "too many non-ACGTU tract candidates in one batch (%llu)",
                                             (unsigned long long) std::max (v.h_ctr->lc[0].n_fix, v.h_ctr->lc[1].n_fix));
  c->n_raw_known = total - (long) v.h_ctr->n_null;
  c->raw_bound = (u64) c->n_raw_known;
  c->bucket_bound = mx;
  c->chunk_bound = v.h_cursors[TJ_P];
  c->n_undefined = (long) v.h_ctr->n_undefined;
  return TJAMD_OK;
}

static int sync_counters (tjamd_counter *c)
{
  int rc = queue_counter_copies (c);
  if (rc) return rc;
  HIPCHK (hipStreamSynchronize (c->stream));
  return apply_counter_copies (c);
}

static void choose_chunk_size (tjamd_counter *c, u64 records)
{ // fixed by the first scan (or reservation) after a reset: at most ~16 k chunks for this many records
  if (c->ch_shift >= 0) return;
  const u64 units = records / (16384ull * TJ_CH0);
  int sft = 3;                                          // a chunk holds more than any one reservation: a partition pass stages 4096 records, partition_log_kernel's TJ_LOGB = 8192
  static_assert ((TJ_CH0 << 3) > (int) TJ_LOGB, "a run of one log block crosses at most one chunk boundary");
  while ((1ull << sft) < units) sft++;
  c->ch_shift = sft;
}

// chunk table with rows of at least need_maxj entries (rows keep their contents)
static int ensure_table (tjamd_counter *c, u64 need_maxj)
{
  if (need_maxj > c->maxj) {
    const u32 nmaxj = (u32) std::max<u64> (need_maxj, (u64) c->maxj + c->maxj / 2);
    void *np = nullptr;
    hipError_t e = hipMalloc (&np, (size_t) TJ_P * nmaxj * 4);
    if (e != hipSuccess) return set_err (TJAMD_ERR_HIP, "hipMalloc of the chunk table failed: %s", hipGetErrorString (e));
    HIPCHK (hipMemsetAsync (np, 0xFF, (size_t) TJ_P * nmaxj * 4, c->stream));
    if (!c->table.p || !c->maxj) {
      hipLaunchKernelGGL (init_table_kernel, dim3 (1), dim3 (TJ_P), 0, c->stream, (u32 *) np, nmaxj, c->d_cursors + TJ_P * TJ_CSTRIDE);
      HIPCHK (hipGetLastError ());
    }
    if (c->table.p) {
      if (c->maxj) {
        hipLaunchKernelGGL (table_relayout_kernel, dim3 (TJ_P), dim3 (256), 0, c->stream, (const u32 *) c->table.p, c->maxj, (u32 *) np, nmaxj);
        HIPCHK (hipGetLastError ());
      }
      HIPCHK (hipStreamSynchronize (c->stream));
      HIPCHK (hipFree (c->table.p));
    }
    c->table.p = np; c->table.cap = (size_t) TJ_P * nmaxj * 4; c->maxj = nmaxj;
  }
  return TJAMD_OK;
}

// room for `add` more raw records (an upper bound), wherever the hash sends them
static int ensure_buckets (tjamd_counter *c, u64 add)
{
  choose_chunk_size (c, add);
  const u64 ch = (u64) TJ_CH0 << c->ch_shift;
  // one chunk per bucket is always claimed ahead of the cursor
  const u64 need_chunks = c->chunk_bound + (add + ch - 1) / ch + 2 * TJ_P;
  c->buckets_clean = false; c->ctr_clean = false;
  const u64 need_maxj = (c->bucket_bound + add + ch - 1) / ch + 3;      // worst case: everything in one bucket
  if (need_chunks >= TJ_NOCHUNK || need_maxj >= (1ull << 31)) return set_err (TJAMD_ERR_CAPACITY, "batch too large for the chunk table");
  int rc = ensure (c->pool, (size_t) need_chunks * ch * c->W * 8, c->stream, std::min<size_t> ((size_t) (c->chunk_bound * ch * c->W * 8), c->pool.cap));
  if (rc) return rc;
  c->pool_chunks = (u32) std::min<u64> (c->pool.cap / (ch * c->W * 8), TJ_NOCHUNK - 1);
  rc = ensure_table (c, need_maxj);
  if (rc) return rc;
  c->chunk_bound = need_chunks;
  c->bucket_bound += add;
  return TJAMD_OK;
}

#define TJ_FIX_CAP (1u << 20)

static int check_scan_args (tjamd_counter *c, int min_tract_size)
{
  if (!c) return set_err (TJAMD_ERR_ARG, "null counter");
  if (min_tract_size < 1 || min_tract_size > 32) return set_err (TJAMD_ERR_ARG, "min_tract_size %d outside [1,32] (reference clamp: src/main.c:186-187)", min_tract_size);
  return TJAMD_OK;
}

// Room for the raw records of about stream_bytes of reads, allocated in one piece instead of by repeated growth (each
// growth is an allocation, a device copy and a synchronisation).  A hint: scans allocate what they need anyway.
extern "C" int tjamd_reserve (tjamd_counter *c, size_t stream_bytes, int min_tract_size)
{
  int rc = check_scan_args (c, min_tract_size);
  if (rc) return rc;
  HIPCHK (hipSetDevice (c->device));
  const u64 records = std::min<u64> ((u64) (stream_bytes / (size_t) std::max (min_tract_size, 2) + 1), ((u64) 4 << 30) / ((u64) c->W * 8));   // (a hint is not worth more than 4 GB)
  choose_chunk_size (c, records);
  const u64 ch = (u64) TJ_CH0 << c->ch_shift;
  const size_t keep = std::min<size_t> (c->pool.cap, (size_t) (c->chunk_bound * ch * c->W * 8));
  rc = ensure (c->pool, (size_t) ((records / ch + 2 * TJ_P + 1) * ch * c->W * 8), c->stream, keep);
  if (rc) return rc;
  c->pool_chunks = (u32) std::min<u64> (c->pool.cap / (ch * c->W * 8), TJ_NOCHUNK - 1);
  c->buckets_clean = c->buckets_clean && c->table.p != nullptr;
  return ensure_table (c, (c->bucket_bound + records + ch - 1) / ch + 3);
}

// one launch of the scan over [d_stream, d_stream + n_bytes) (16-byte aligned, starts and ends on read boundaries)
static int scan_device_piece (tjamd_counter *c, const void *d_stream, size_t n_bytes, int min_tract_size, bool first, bool last)
{
  int rc = TJAMD_OK;
  if (n_bytes < 64 && d_stream != c->stage.p) {             // the kernels read whole 16-byte chunks: give tiny streams room
    rc = ensure (c->stage, 256, c->stream);
    if (rc) return rc;
    HIPCHK (hipMemcpyAsync (c->stage.p, d_stream, n_bytes, hipMemcpyDeviceToDevice, c->stream));
    d_stream = c->stage.p;
  }
  const int mprime = std::max (min_tract_size, 2);          // a tract needs two equal bytes: m = 1 behaves as m = 2
  // tracts are disjoint runs of >= m' bytes: at most n/m' records come out of this batch
  const u64 bound = (u64) ((double) (n_bytes / (size_t) mprime + 1) * c->slack);
  const long n_tiles = (long) ((n_bytes + TJ_SB_TILE - 1) / TJ_SB_TILE);
  const int grid = (int) std::min<long> (n_tiles, (long) c->n_cu * TJ_SB_WG_PER_CU);
  rc = ensure_buckets (c, bound);
  c->raw_bound += (u64) (n_bytes / (size_t) mprime) + 1u;
  if (!rc) rc = ensure (c->fix, (size_t) TJ_FIX_CAP * sizeof (FixEntry), c->stream);
  // fast kernel: tiles of FK_OWN tract starts, two workgroups resident per CU; the list of the tiles it leaves to the generic
  // kernel (every one of them at worst), which that kernel covers with ceil (FK_OWN / TJ_SB_TILE) of its own tiles each
  const long n_ftiles = (long) ((n_bytes + FK_OWN - 1) / FK_OWN);
  const int fgrid = (int) std::min<long> (n_ftiles, (long) c->n_cu * FK_WG_PER_CU);
  const int lgrid = (int) std::min<long> (n_ftiles * ((FK_OWN + TJ_SB_TILE - 1) / TJ_SB_TILE), (long) c->n_cu * TJ_SB_WG_PER_CU);
  if (!rc && c->fast_mode) rc = ensure (c->slow, (size_t) n_ftiles * 4 + 64, c->stream);
  if (rc) return rc;
  const uint8_t *seq = (const uint8_t *) d_stream;
  const Buckets BK = make_buckets (c);
  FixEntry *fix = (FixEntry *) c->fix.p;
  const int par = (int) (c->scan_seq++ & 1u);            // per-launch counters are double-buffered (DevCounters::lc)
  if (first) HIPCHK (c->timer[T_SCAN].begin (c->stream));
  const TileSrc plain = {nullptr, 0};
  // (TATAJUBA_AMD_SCAN_GRID: the launches below take at most that many workgroups; the storage above stays sized for the full grids)
  auto capped = [c] (long g) { return (unsigned) (c->scan_grid_cap >= 1 ? std::min<long> (g, (long) c->scan_grid_cap) : g); };
  // (the fast kernel counts tiles and bytes in 32 bits: a piece that could not be cut below 2 GiB -- one read longer
  // than that -- is left to the general kernel)
  const bool use_fast = c->fast_mode && n_bytes < ((size_t) 1 << 31) - (1u << 20);
  // one-word records (k <= 12): the fast kernel appends to a log sized for the worst case (a tract every m' bytes; every
  // workgroup leaves at most two blocks partly filled), partition_log_kernel distributes it over the buckets
  const bool use_log = use_fast && c->W <= c->log_mode;
  LogSpace LG = {nullptr, nullptr, nullptr, 0u};
  const int fgrid_log = (int) std::min<long> (n_ftiles, (long) c->n_cu * FK_LOG_WG_PER_CU);
  if (use_log) {
    // (a workgroup with n records has taken at most n / TJ_LOGB + 3 blocks: the one being filled and up to two ahead of it)
    const u64 n_blocks = ((bound * (u64) c->W) >> TJ_LOGB_SHIFT) + 3ull * (u64) fgrid_log + 8ull;      // (a block is TJ_LOGB words: TJ_LOGB / W records)
    rc = ensure (c->log, (size_t) (((n_blocks << TJ_LOGB_SHIFT) + 64ull * (u64) fgrid_log) * 8ull), c->stream);
    if (!rc && (size_t) (n_blocks + 2) * 4 > c->logmeta.cap) {
      rc = ensure (c->logmeta, (size_t) (n_blocks + 2) * 4 * 2, c->stream);
      c->log_next_clean[0] = c->log_next_clean[1] = false;
    }
    if (rc) return rc;
    u32 *meta = (u32 *) c->logmeta.p;
    if (!c->log_next_clean[par]) HIPCHK (hipMemsetAsync (meta + par, 0, 4, c->stream));
    LG.log = (u64 *) c->log.p; LG.next = meta + par; LG.next_other = meta + (par ^ 1); LG.count = meta + 2; LG.n_blocks = (u32) n_blocks;
    c->log_next_clean[par] = false; c->log_next_clean[par ^ 1] = true;
  }
  with_width (c->W, [&] (auto w) {
    constexpr int W = decltype (w)::value;
    if (use_fast) {
      // the fast kernel takes every tile it can vouch for and lists the others; the generic kernel then works through the list
      if (use_log) {
        if constexpr (W <= 2)                             // (the log form exists for W <= 2 only: log_mode is 2 at most)
          hipLaunchKernelGGL ((scan_fast_kernel<W, true>), dim3 (capped (fgrid_log)), dim3 (FK_BLOCK), 0, c->stream, seq, (long) n_bytes, n_ftiles, c->k, mprime, BK, c->d_ctr,
                              (u32 *) c->slow.p, par, c->fast_mode == 2 ? 1 : 0, LG);
      }
      else
        hipLaunchKernelGGL (scan_fast_kernel<W>, dim3 (capped (fgrid)), dim3 (FK_BLOCK), 0, c->stream, seq, (long) n_bytes, n_ftiles, c->k, mprime, BK, c->d_ctr,
                            (u32 *) c->slow.p, par, c->fast_mode == 2 ? 1 : 0, LG);
      const TileSrc listed = {(const u32 *) c->slow.p, (long) FK_OWN};
      hipLaunchKernelGGL (scan_bins_kernel<W>, dim3 (capped (lgrid)), dim3 (TJ_SB_BLOCK), 0, c->stream, seq, (long) n_bytes, 0l, c->k, mprime, BK, c->d_ctr, fix, (u32) TJ_FIX_CAP, par, listed);
    }
    else {
      hipLaunchKernelGGL (scan_bins_kernel<W>, dim3 (capped (grid)), dim3 (TJ_SB_BLOCK), 0, c->stream, seq, (long) n_bytes, n_tiles, c->k, mprime, BK, c->d_ctr, fix, (u32) TJ_FIX_CAP, par, plain);
      hipLaunchKernelGGL (nrun_fixup_bins_kernel<W>, dim3 (64), dim3 (256), 0, c->stream, seq, (long) n_bytes, c->k, mprime, BK, c->d_ctr, (const FixEntry *) fix, (u32) TJ_FIX_CAP, par);
    }
  });
  HIPCHK (hipGetLastError ());
  if (last) HIPCHK (c->timer[T_SCAN].end (c->stream));
  if (first) c->n_piece_ev = 0;
  const bool mid_events = use_log && !last && c->n_piece_ev < TJ_PIECE_EVENTS;
  if (mid_events) {
    const int i = c->n_piece_ev;
    if (!c->ev_pa[i]) { HIPCHK (hipEventCreate (&c->ev_pa[i])); HIPCHK (hipEventCreate (&c->ev_pb[i])); }
    HIPCHK (hipEventRecord (c->ev_pa[i], c->stream));
  }
  if (use_log) {
    with_width (c->W, [&] (auto w) {
      constexpr int W = decltype (w)::value;
      if constexpr (W <= 2) hipLaunchKernelGGL (partition_log_kernel<W>, dim3 (capped ((long) c->n_cu * PL_WG_PER_CU)), dim3 (PL_BLOCK), 0, c->stream, LG, BK, c->d_ctr, c->k);
    });
    HIPCHK (hipGetLastError ());
  }
  if (mid_events) { HIPCHK (hipEventRecord (c->ev_pb[c->n_piece_ev], c->stream)); c->n_piece_ev++; }
  if (last) { HIPCHK (hipEventRecord (c->ev_p1, c->stream)); c->part_timed = use_log; }
  c->timer[T_SCAN].timed = true;
  c->last_scan_launches = first ? 1 : c->last_scan_launches + 1;
  c->status = -1;
  return TJAMD_OK;
}

// A stream is scanned in one launch up to 1.5 x TJ_SCAN_PIECE_TARGET bytes.  A longer one goes piece by piece, each piece cut
// after a read delimiter that sits on the last byte of a 16-byte line (so that the next piece starts aligned; with reads
// of any length one turns up within a few reads), and the exact record counts are fetched between pieces: the device
// storage then follows what the reads really contain instead of the worst case of the whole stream (n / m' records).

__global__ __launch_bounds__ (1024)
void find_cut_kernel (const uint8_t *__restrict__ seq, unsigned long long first_from, unsigned long long step, unsigned long long n, unsigned long long *out)
{ // out[b] = smallest p >= first_from + b * step with p % 16 == 15 and seq[p] == '\n', or ~0 (one workgroup per cut)
  __shared__ unsigned long long best;
  const unsigned long long from = first_from + (unsigned long long) blockIdx.x * step;
  if (threadIdx.x == 0) best = ~0ull;
  __syncthreads ();
  for (unsigned long long base = from & ~15ull; base < n; base += 1024ull * 16ull) {
    const unsigned long long p = base + 16ull * threadIdx.x + 15ull;
    if (p >= from && p < n && seq[p] == (uint8_t) '\n') atomicMin (&best, p);
    __syncthreads ();
    if (best != ~0ull) break;
    __syncthreads ();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = best;
}

extern "C" int tjamd_scan_device (tjamd_counter *c, const void *d_stream, size_t n_bytes, int min_tract_size)
{
  int rc = check_scan_args (c, min_tract_size);
  if (rc) return rc;
  if (n_bytes == 0) return TJAMD_OK;
  if (!d_stream || ((uintptr_t) d_stream & 15u)) return set_err (TJAMD_ERR_ARG, "device stream pointer must be non-null and 16-byte aligned");
  HIPCHK (hipSetDevice (c->device));
  const size_t piece_target = c->piece_target, piece_max = piece_target + piece_target / 2;
  if (n_bytes <= piece_max) return scan_device_piece (c, d_stream, n_bytes, min_tract_size, true, true);
  const uint8_t *seq = (const uint8_t *) d_stream;
  // every piece is cut near a multiple of the target: the cuts do not depend on each other, so they are all looked for
  // by one launch and fetched with one copy (per piece that would be a kernel, a copy and a synchronisation of 25 us)
  const size_t n_cuts = (n_bytes - 1) / piece_target;    // candidates at piece_target, 2 piece_target, ...
  std::vector<unsigned long long> cuts (n_cuts);
  rc = ensure (c->prefix, 64 + 8 * n_cuts, c->stream);
  if (rc) return rc;
  hipLaunchKernelGGL (find_cut_kernel, dim3 ((unsigned) n_cuts), dim3 (1024), 0, c->stream, seq, (unsigned long long) piece_target, (unsigned long long) piece_target,
                      (unsigned long long) n_bytes, (unsigned long long *) c->prefix.p);
  HIPCHK (hipMemcpyAsync (cuts.data (), c->prefix.p, 8 * n_cuts, hipMemcpyDeviceToHost, c->stream));
  HIPCHK (hipStreamSynchronize (c->stream));
  size_t off = 0, next_cut = 0;
  bool first = true;
  while (off < n_bytes) {
    size_t end = n_bytes;
    if (n_bytes - off > piece_max) {
      // the next cut that makes a piece of at least half the target (cuts come in increasing order, about a target apart)
      while (next_cut < n_cuts && (cuts[next_cut] == ~0ull || cuts[next_cut] + 1 < off + piece_target / 2)) next_cut++;
      if (next_cut < n_cuts && cuts[next_cut] + 1 < n_bytes) end = (size_t) cuts[next_cut] + 1;
    }
    rc = scan_device_piece (c, seq + off, end - off, min_tract_size, first, end == n_bytes);
    if (rc) return rc;
    if (end < n_bytes && (rc = sync_counters (c))) return rc;     // exact counts: the next piece adds its own worst case to them
    off = end;
    first = false;
  }
  return TJAMD_OK;
}

extern "C" int tjamd_scan_host (tjamd_counter *c, const void *h_stream, size_t n_bytes, int min_tract_size)
{
  if (!c) return set_err (TJAMD_ERR_ARG, "null counter");
  if (n_bytes == 0) return TJAMD_OK;
  if (!h_stream) return set_err (TJAMD_ERR_ARG, "null host stream");
  HIPCHK (hipSetDevice (c->device));
  int rc = ensure (c->stage, (n_bytes + 255) & ~(size_t) 255, c->stream);
  if (rc) return rc;
  HIPCHK (hipMemcpyAsync (c->stage.p, h_stream, n_bytes, hipMemcpyHostToDevice, c->stream));
  return tjamd_scan_device (c, c->stage.p, n_bytes, min_tract_size);
}

extern "C" long tjamd_scan_host_located (tjamd_counter *c, const void *h_stream, size_t n_bytes, int min_tract_size,
                                          tjamd_located_record *out, long capacity)
{ // min_tract_size == 0: every isolated base instead of tracts (reference: update_hopo_counter_from_seq_all_monomers)
  int rc = (min_tract_size == 0 && c) ? TJAMD_OK : check_scan_args (c, min_tract_size);
  if (rc) return -rc;
  if (n_bytes == 0) return 0;
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  const int mprime = min_tract_size == 0 ? 0 : std::max (min_tract_size, 2);
  const long bound = (long) (n_bytes / (size_t) (mprime ? mprime : 1)) + 1;
  rc = ensure (c->stage, (n_bytes + 255) & ~(size_t) 255, c->stream);
  if (!rc) rc = ensure (c->loc, (size_t) bound * 32, c->stream);
  if (!rc) rc = ensure (c->fix, (size_t) TJ_FIX_CAP * sizeof (FixEntry), c->stream);
  if (rc) return -rc;
  if (hipMemcpyAsync (c->stage.p, h_stream, n_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemsetAsync (c->d_lctr, 0, sizeof (DevCounters), c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "copy to device failed");
  const long n_tiles = (long) ((n_bytes + 4095) / 4096);
  hipLaunchKernelGGL (scan_list_kernel, dim3 ((unsigned) std::min<long> (n_tiles, 2048)), dim3 (256), 0, c->stream, (const uint8_t *) c->stage.p, (long) n_bytes,
                      n_tiles, c->k, mprime, (u64 *) c->loc.p, (u64) bound, c->d_lctr, (FixEntry *) c->fix.p, (u32) TJ_FIX_CAP, 0);
  hipLaunchKernelGGL (nrun_fixup_list_kernel, dim3 (64), dim3 (256), 0, c->stream, (const uint8_t *) c->stage.p, (long) n_bytes, c->k, mprime,
                      (u64 *) c->loc.p, (u64) bound, c->d_lctr, (const FixEntry *) c->fix.p, (u32) TJ_FIX_CAP, 0);
  if (hipGetLastError () != hipSuccess) return -set_err (TJAMD_ERR_HIP, "located scan launch failed");
  if (hipMemcpyAsync (c->h_ctr, c->d_lctr, sizeof (DevCounters), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize (c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "located scan failed: %s", hipGetErrorString (hipGetLastError ()));
  const DevCounters h = *c->h_ctr;
  if (h.overflow || h.fix_overflow) return -set_err (TJAMD_ERR_CAPACITY, "located scan overflow");
  c->n_undefined += (long) h.n_undefined;
  const long n = (long) h.n_rec;
  if (n > capacity) return -set_err (TJAMD_ERR_CAPACITY, "located scan produced %ld records, caller capacity %ld", n, capacity);
  if (n) {
    if (hipMemcpy (out, c->loc.p, (size_t) n * 32, hipMemcpyDeviceToHost) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "download failed");
    std::sort (out, out + n, [] (const tjamd_located_record &a, const tjamd_located_record &b) { return a.pos < b.pos; });
  }
  return n;
}

extern "C" long tjamd_raw_count (tjamd_counter *c)
{
  if (!c) return -set_err (TJAMD_ERR_ARG, "null counter");
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  int rc = sync_counters (c);
  return rc ? -rc : c->n_raw_known;
}

// diagnostic: records per hash bucket after a synchronisation (not part of the public header)
extern "C" long tjamd_debug_bucket_counts (tjamd_counter *c, unsigned *out, int n)
{
  if (tjamd_raw_count (c) < 0) return -1;
  for (int b = 0; b < n && b < TJ_P; b++) out[b] = c->h_cursors[b];
  return TJ_P;
}

// diagnostic (tests, tools): tiles the fast kernel of the last scan launch handed over to the generic kernel
extern "C" long tjamd_debug_slow_tiles (tjamd_counter *c)
{
  if (tjamd_raw_count (c) < 0) return -1;
  return (long) c->h_ctr->lc[(c->scan_seq - 1u) & 1u].n_slow;
}

extern "C" long tjamd_undefined_runs (tjamd_counter *c)
{
  if (tjamd_raw_count (c) < 0) return -1;
  return c->n_undefined;
}

extern "C" long tjamd_download_raw (tjamd_counter *c, tjamd_record *out, long capacity)
{
  long n = tjamd_raw_count (c);
  if (n < 0) return n;
  if (n > capacity) return -set_err (TJAMD_ERR_CAPACITY, "%ld raw records, caller capacity %ld", n, capacity);
  if (n == 0) return 0;
  int rc = ensure (c->prefix, 64, c->stream);
  if (!rc) rc = ensure (c->rawlist, (size_t) n * 24, c->stream);
  if (rc) return -rc;
  if (hipMemsetAsync (c->prefix.p, 0, 8, c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "memset failed");
  const Buckets BK = make_buckets (c);
  with_width (c->W, [&] (auto w) {
    hipLaunchKernelGGL (unpack_buckets_kernel<decltype (w)::value>, dim3 (TJ_P), dim3 (256), 0, c->stream, BK, c->k, (u64 *) c->rawlist.p, (u64) n, (u64 *) c->prefix.p);
  });
  u64 n_out = 0;
  if (hipGetLastError () != hipSuccess || hipStreamSynchronize (c->stream) != hipSuccess ||
      hipMemcpy (&n_out, c->prefix.p, 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy (out, c->rawlist.p, (size_t) n * 24, hipMemcpyDeviceToHost) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "raw download failed");
  if ((long) n_out != n) return -set_err (TJAMD_ERR_STATE, "raw download found %llu records, cursors say %ld", (unsigned long long) n_out, n);
  return n;
}

extern "C" int tjamd_upload_raw (tjamd_counter *c, const hopo_element *elems, long n)
{
  if (!c || (n && !elems) || n < 0) return set_err (TJAMD_ERR_ARG, "bad arguments");
  if (n == 0) return TJAMD_OK;
  HIPCHK (hipSetDevice (c->device));
  int rc = sync_counters (c);
  if (!rc) rc = ensure_buckets (c, (u64) n);
  c->raw_bound += (u64) n;
  if (!rc) rc = ensure (c->stage, (size_t) n * 40, c->stream);
  if (rc) return rc;
  HIPCHK (hipMemcpyAsync (c->stage.p, elems, (size_t) n * 40, hipMemcpyHostToDevice, c->stream));
  const unsigned grid = (unsigned) std::min<long> ((n + 255) / 256, 2048);
  const Buckets BK = make_buckets (c);
  with_width (c->W, [&] (auto w) {
    hipLaunchKernelGGL (bin_elems_kernel<decltype (w)::value>, dim3 (grid), dim3 (256), 0, c->stream, (const u64 *) c->stage.p, n, c->k, BK, c->d_ctr);
  });
  HIPCHK (hipGetLastError ());
  c->status = -1;
  return sync_counters (c);
}

// ---- device-wide exclusive scan ------------------------------------------------------------------------------------

static int exclusive_scan (tjamd_counter *c, const u32 *in, u32 *out, long n, u32 *total_out, u32 *tmp, size_t tmp_words)
{ // tmp: scratch for block sums of every level (n/4096 + n/4096^2 + ... + 2 words)
  if (n <= 0) return TJAMD_OK;
  long nblk = (n + SC_ITEMS - 1) / SC_ITEMS;
  if (nblk == 1) {
    hipLaunchKernelGGL (scan_apply_kernel, dim3 (1), dim3 (256), 0, c->stream, in, out, n, (const u32 *) nullptr, total_out);
    HIPCHK (hipGetLastError ());
    return TJAMD_OK;
  }
  if ((size_t) nblk > tmp_words) return set_err (TJAMD_ERR_STATE, "scan scratch too small");
  hipLaunchKernelGGL (scan_reduce_kernel, dim3 ((unsigned) nblk), dim3 (256), 0, c->stream, in, n, tmp);
  HIPCHK (hipGetLastError ());
  int rc = exclusive_scan (c, tmp, tmp, nblk, nullptr, tmp + nblk, tmp_words - (size_t) nblk);
  if (rc) return rc;
  hipLaunchKernelGGL (scan_apply_kernel, dim3 ((unsigned) nblk), dim3 (256), 0, c->stream, in, out, n, (const u32 *) tmp, total_out);
  HIPCHK (hipGetLastError ());
  return TJAMD_OK;
}
// the same in the counter's own scan scratch, which the caller has sized with scan_tmp_words
static int exclusive_scan (tjamd_counter *c, const u32 *in, u32 *out, long n, u32 *total_out) { return exclusive_scan (c, in, out, n, total_out, (u32 *) c->scan_tmp.p, c->scan_tmp.cap / 4); }

static size_t scan_tmp_words (long n)
{
  size_t w = 8;
  while (n > SC_ITEMS) { n = (n + SC_ITEMS - 1) / SC_ITEMS; w += (size_t) n; }
  return w;
}

static int radix_sort_records (tjamd_counter *c, u64 *&a, u64 *&b, long n)
{ // a: input (sorted result ends in a), b: scratch of the same size
  const int passes = key_passes (c->k);
  const int nblk = (int) ((n + RS_ITEMS - 1) / RS_ITEMS);
  const long nh = 256l * nblk;
  int rc = ensure (c->hist, (size_t) nh * 4, c->stream);
  if (!rc) rc = ensure (c->scan_tmp, std::max (scan_tmp_words (nh), scan_tmp_words (n)) * 4, c->stream);
  if (rc) return rc;
  for (int p = 0; p < passes; p++) {
    hipLaunchKernelGGL (radix_count_kernel, dim3 (nblk), dim3 (256), 0, c->stream, (const u64 *) a, n, p, c->k, (u32 *) c->hist.p, nblk);
    HIPCHK (hipGetLastError ());
    rc = exclusive_scan (c, (const u32 *) c->hist.p, (u32 *) c->hist.p, nh, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL (radix_scatter_kernel, dim3 (nblk), dim3 (256), 0, c->stream, (const u64 *) a, b, n, p, c->k, (const u32 *) c->hist.p, nblk);
    HIPCHK (hipGetLastError ());
    std::swap (a, b);
  }
  return TJAMD_OK;
}

static unsigned grid_for (long n) { return (unsigned) std::max<long> (1, std::min<long> ((n + 255) / 256, 4096)); }

// ---- finalise steps 3-4 + coverage, two ways --------------------------------------------------------------------


// radix path: stable LSD sort, then heads / scans / decisions as separate kernels (any bin occupancy, any size)
static int finalise_radix (tjamd_counter *c, long n1, int min_coverage)
{
  int rc = ensure (c->alt, (size_t) n1 * 24, c->stream);
  if (!rc) rc = ensure (c->flags, (size_t) n1 * 4, c->stream);
  if (!rc) rc = ensure (c->segid, (size_t) n1 * 4, c->stream);
  if (!rc) rc = ensure (c->headpos, (size_t) n1 * 4, c->stream);
  if (!rc) rc = ensure (c->keep, (size_t) n1 * 4, c->stream);
  if (!rc) rc = ensure (c->outpos, (size_t) n1 * 4, c->stream);
  if (!rc) rc = ensure (c->scan_tmp, scan_tmp_words (n1) * 4, c->stream);
  if (rc) return rc;
  u64 *a = (u64 *) c->kept.p, *b = (u64 *) c->alt.p;
  rc = radix_sort_records (c, a, b, n1);
  if (rc) return rc;
  if (a != (u64 *) c->kept.p) std::swap (c->kept, c->alt);

  // step 4: contexts deep enough get an index range (reference :388-404)
  const u64 *kept = (const u64 *) c->kept.p;
  u32 *flags = (u32 *) c->flags.p, *segid = (u32 *) c->segid.p, *headpos = (u32 *) c->headpos.p;
  u32 *keep = (u32 *) c->keep.p, *outpos = (u32 *) c->outpos.p;
  hipLaunchKernelGGL (seg_heads_kernel, dim3 (grid_for (n1)), dim3 (256), 0, c->stream, kept, n1, flags, 1);
  HIPCHK (hipGetLastError ());
  rc = exclusive_scan (c, flags, segid, n1, &c->d_fin->n_ctx);
  if (rc) return rc;
  hipLaunchKernelGGL (seg_headpos_kernel, dim3 (grid_for (n1)), dim3 (256), 0, c->stream, (const u32 *) flags, (const u32 *) segid, n1, headpos);
  HIPCHK (hipGetLastError ());
  hipLaunchKernelGGL (ctx_decide_kernel, dim3 (grid_for (n1)), dim3 (256), 0, c->stream, kept, n1, (const u32 *) headpos,
                      (const u32 *) &c->d_fin->n_ctx, min_coverage, keep);
  HIPCHK (hipGetLastError ());
  HIPCHK (hipMemcpyAsync (c->h_fin, c->d_fin, sizeof (FinCounts), hipMemcpyDeviceToHost, c->stream));
  HIPCHK (hipStreamSynchronize (c->stream));
  const long n_ctx = c->h_fin->n_ctx;
  rc = exclusive_scan (c, keep, outpos, n_ctx, &c->d_fin->n_idx);
  if (!rc) rc = ensure (c->idx_i, (size_t) n_ctx * 4, c->stream);
  if (!rc) rc = ensure (c->idx_f, (size_t) n_ctx * 4, c->stream);
  if (rc) return rc;
  hipLaunchKernelGGL (ctx_write_kernel, dim3 (grid_for (n_ctx)), dim3 (256), 0, c->stream, n1, (const u32 *) headpos, (const u32 *) &c->d_fin->n_ctx,
                      (const u32 *) keep, (const u32 *) outpos, (int *) c->idx_i.p, (int *) c->idx_f.p);
  HIPCHK (hipGetLastError ());

  // coverage (reference :419-438)
  const int log2t = cov_table_bits (n1);
  const long t = 1l << log2t;
  rc = ensure (c->cov, (size_t) t * 8, c->stream);
  if (rc) return rc;
  u64 *ctab = (u64 *) c->cov.p;
  HIPCHK (hipMemsetAsync (c->cov.p, 0, (size_t) t * 8, c->stream));
  hipLaunchKernelGGL (set_int_kernel, dim3 (1), dim3 (1), 0, c->stream, &c->d_fin->coverage, INT_MIN);
  hipLaunchKernelGGL (cov_insert_kernel, dim3 (grid_for (2 * n1)), dim3 (256), 0, c->stream, kept, n1, ctab, log2t);
  HIPCHK (hipGetLastError ());
  hipLaunchKernelGGL (cov_max_kernel, dim3 (std::min<unsigned> (grid_for (t), 256u)), dim3 (256), 0, c->stream, (const u64 *) ctab, t, &c->d_fin->coverage);
  HIPCHK (hipGetLastError ());
  if ((rc = end_fin_interval (c, c->stream))) return rc;
  HIPCHK (hipMemcpyAsync (c->h_fin, c->d_fin, sizeof (FinCounts), hipMemcpyDeviceToHost, c->stream));
  HIPCHK (hipStreamSynchronize (c->stream));
  return TJAMD_OK;
}

// binned path: kept (n1 records, any order) -> sorted kept, idx_i / idx_f, FinCounts{n_idx, coverage}; one host
// synchronisation at the end.  If a bin turns out too full every kernel after the bin scan does nothing, kept stays as
// it was and FinCounts::sort_fallback comes back set.
// n1 > 0: the kept count, known.  n1 == 0: not fetched yet -- the kernels take their sizes from the device-side plan
// (plan_tail has run), the buffers hold `cap` records, and the caller looks at what came of it after the one
// synchronisation at the end (finalise_speculative_ok).
static int finalise_binned (tjamd_counter *c, long n1, int min_coverage, long cap = 0, bool wait = true)
{
  const bool planned = n1 == 0;
  // (begun, not waited for, and a second stream is there: the step goes to it, behind what the counter's stream holds so far)
  // (the library's side stream unless the caller named a stream, or none; taken only here, where it is first needed)
  hipStream_t other = nullptr;
  if (planned && !wait) other = c->order_mode == tjamd_counter::ORDER_GIVEN ? c->order_stream : c->order_mode == tjamd_counter::ORDER_SIDE ? side_stream_acquire (c) : nullptr;
  const bool aside = other != nullptr && other != c->stream;
  const hipStream_t st = aside ? other : c->stream;
  c->order_path |= aside ? 1u : planned ? 4u : 2u;
  const FinPlan *plan = planned ? &c->d_state->plan : nullptr;
  if (planned) n1 = cap;                                // (sizes everything below; the kernels use the plan's numbers)
  const int nbits = bin_bits_for (n1, c->k);
  const int nbins = planned ? BS_MAXBINS : 1 << nbits;  // (planned: the layout of binctx / binout must not depend on the count)
  // (planned: the table is allocated for the capacity's hash table, the kernels take their numbers from the plan -- a
  // table addressed by the key is never larger than that, see cov_plan_bits)
  int cov_direct = 0;
  const int log2t = planned ? cov_table_bits (n1) : cov_plan_bits (n1, c->k, &cov_direct);
  const long t = 1l << log2t;
  // the aggregation has counted the kept records into the finest bins (finalise_queue): no counting pass
  const bool fused = planned && c->bins_counted;
  c->bins_counted = false;
  int rc = ensure (c->alt, (size_t) n1 * 24, c->stream);
  if (!rc && !c->bins.p) { rc = ensure (c->bins, (size_t) (BS_MAXBINS + 1) * 4, c->stream); c->bins_zeroed = false; }
  if (!rc) rc = ensure (c->binstart, (size_t) (nbins + 1) * 4, c->stream);
  if (!rc) rc = ensure (c->binctx, ((size_t) nbins * 3 + 1) * 4, c->stream);    // (binctx, binout, then the list of fuller bins and its count)
  if (!rc) rc = ensure (c->headpos, (size_t) n1 * 4, c->stream);
  if (!rc) rc = ensure (c->outpos, (size_t) n1 * 4, c->stream);
  if (!rc) rc = ensure (c->idx_i, (size_t) n1 * 4, c->stream);
  if (!rc) rc = ensure (c->idx_f, (size_t) n1 * 4, c->stream);
  if (!rc) rc = ensure (c->cov, (size_t) t * 8, c->stream);
  if (rc) return rc;
  u32 *bins = (u32 *) c->bins.p, *binstart = (u32 *) c->binstart.p, *binctx = (u32 *) c->binctx.p, *binout = binctx + nbins, *full = binout + nbins;
  u32 *tstart = (u32 *) c->headpos.p, *tend = (u32 *) c->outpos.p;
  u64 *ctab = (u64 *) c->cov.p;
  if (!fused && !c->bins_zeroed) HIPCHK (hipMemsetAsync (bins, 0, (size_t) BS_MAXBINS * 4, c->stream));
  c->bins_zeroed = false;
  if (aside) { HIPCHK (hipEventRecord (c->ev_agg, c->stream)); HIPCHK (hipStreamWaitEvent (st, c->ev_agg, 0)); }
  // (planned: the grids are sized for a typical kept count, not for the buffers' capacity -- the kernels stride)
  const unsigned g1 = planned ? std::min<unsigned> (grid_for (n1), 2048u) : grid_for (n1);
  if (!fused) hipLaunchKernelGGL (bin_count_kernel, dim3 (g1), dim3 (256), 0, st, (const u64 *) c->kept.p, n1, c->k, nbits, bins,
                                  (uint4 *) c->cov.p, (long) (t / 2), 0, plan);
  hipLaunchKernelGGL (bin_scan_kernel, dim3 (1), dim3 (WGS_THREADS), 0, st, bins, nbins, binstart, c->bin_rank_max, c->d_fin, plan, full);
  hipLaunchKernelGGL (bin_scatter_kernel, dim3 (g1), dim3 (256), 0, st, (const u64 *) c->kept.p, (u64 *) c->alt.p, n1, c->k, nbits, bins, plan,
                      fused ? (uint4 *) c->cov.p : (uint4 *) nullptr);
  hipLaunchKernelGGL (bin_sort_index_kernel, dim3 ((unsigned) std::min (nbins + 1, 16384)), dim3 (64), 0, st,
                      (const u64 *) c->alt.p, (u64 *) c->kept.p, (const u32 *) binstart, nbins, (const FinCounts *) c->d_fin, min_coverage,
                      ctab, log2t, binctx, tstart, tend, full, plan, cov_direct);
  // (the bins of more than 64 records that the launch above has listed; few or none: a small grid that strides)
  hipLaunchKernelGGL (bin_sort_full_kernel, dim3 ((unsigned) std::min (nbins, BSF_GRID)), dim3 (64), 0, st,
                      (const u64 *) c->alt.p, (u64 *) c->kept.p, (const u32 *) binstart, nbins, (const FinCounts *) c->d_fin, min_coverage,
                      ctab, log2t, binctx, tstart, tend, full, plan, cov_direct);
  hipLaunchKernelGGL (bin_ctx_scan_kernel, dim3 (1), dim3 (WGS_THREADS), 0, st, (const u32 *) binctx, nbins, binout, c->d_fin, plan);
  hipLaunchKernelGGL (bin_ctx_write_kernel, dim3 (256), dim3 (256), 0, st, (const u32 *) binstart, (const u32 *) binctx, (const u32 *) binout, nbins,
                      (const u32 *) tstart, (const u32 *) tend, (int *) c->idx_i.p, (int *) c->idx_f.p, (const u64 *) ctab, t, c->d_fin, plan);
  HIPCHK (hipGetLastError ());
  if ((rc = end_fin_interval (c, st))) return rc;
  if (planned) HIPCHK (hipMemcpyAsync (c->h_state, c->d_state, sizeof (DevState), hipMemcpyDeviceToHost, st));   // (counts of the sample, plan, results: one copy)
  else HIPCHK (hipMemcpyAsync (c->h_fin, c->d_fin, sizeof (FinCounts), hipMemcpyDeviceToHost, c->stream));
  if (wait) HIPCHK (hipStreamSynchronize (c->stream));
  else HIPCHK (hipEventRecord (c->ev_done, st));
  return TJAMD_OK;
}

// A finalise in two halves.  finalise_queue queues everything (one stream, no host synchronisation when the ordering step can
// be planned on the device); finalise_collect waits for the counts -- after tjamd_finalise_begin an event, not the stream:
// what the caller has queued behind (the next sample's scan on another counter of the same stream) runs on -- and finishes
// the bookkeeping.  c->fin carries what the second half needs to know of the first.
// wait: the ordering step planned ahead ends with a synchronisation of the stream (tjamd_finalise), not with ev_done
static int finalise_queue (tjamd_counter *c, int remove_biased, int min_coverage, bool wait)
{
  if (!c) return set_err (TJAMD_ERR_ARG, "null counter");
  HIPCHK (hipSetDevice (c->device));
  FinCarry &f = c->fin;
  f = FinCarry {FIN_IDLE, remove_biased, min_coverage};   // (idle until all of it is queued: a failure below leaves nothing begun)
  // The raw count sizes the kept list.  A survivor stands for at least two raw records (both strands seen, or a count
  // above one), so half of the host's running upper bound of the raw count is a safe capacity: unless that is a lot of
  // memory, the aggregation is launched without first asking the device (one host round trip less) and the exact
  // counts and error flags, copied in stream order before the buckets are cleared, are looked at afterwards.
  c->n_kept = 0; c->n_idx = 0; c->coverage = 0; c->timer[T_FIN].timed = false; c->order_path = 0;
  f.speculative = (c->raw_bound / 2 + 1) * 24 <= (8ull << 30);
  f.kept_cap = c->raw_bound / 2 + 1;
  int rc = TJAMD_OK;
  if (!f.speculative) {
    rc = sync_counters (c);
    if (rc) return rc;
    if (c->n_raw_known == 0) { f.state = FIN_SETTLED; return finalise_status (c, nullptr, 1); }     // reference: src/hopo_counter.c:345-349
    if (c->n_raw_known >= (1l << 31)) return set_err (TJAMD_ERR_CAPACITY, "%ld raw records exceed the reference's int n_elem", c->n_raw_known);
    f.kept_cap = (u64) c->n_raw_known / 2 + 1;
  }

  // steps 1-2: per-bucket hash aggregation + filter (reference :351-374)
  rc = ensure (c->kept, (size_t) f.kept_cap * 24, c->stream);
  if (!rc) rc = ensure (c->ovf, c->pool.cap, c->stream);   // second pool for the aggregation's leftover rounds
  if (rc) return rc;
  HIPCHK (c->timer[T_FIN].begin (c->stream));
  const Buckets BK = make_buckets (c);
  // The ordering step is launched right behind the aggregation, sized on the device (plan_tail, by the aggregation's last
  // workgroup) for up to kept_cap / 8 records -- a sample keeps a per cent or so of its raw records -- so that the whole
  // finalise has one host round trip; if more were kept, its kernels do nothing and the step is run again by
  // finalise_collect with the count in hand.
  long plan_cap = (long) std::min<u64> (f.kept_cap, std::max<u64> (f.kept_cap / 8, 1u << 16));
  if (const char *pc = getenv ("TATAJUBA_AMD_PLAN_CAP")) plan_cap = std::max (1l, std::min (plan_cap, atol (pc)));     // (tests: make the second attempt happen)
  f.plan_ahead = f.speculative && getenv ("TATAJUBA_AMD_NO_PLAN") == nullptr;
  FinPlan *const d_plan = f.plan_ahead ? &c->d_state->plan : nullptr;
  // with the ordering step planned ahead the aggregation counts what it keeps into the finest bins of that step
  // (clear_buckets_kernel, next on the stream, sums them to the bins the plan asks for and zeroes them again)
  u32 *fine = nullptr;
  if (f.plan_ahead && getenv ("TATAJUBA_AMD_NO_FUSED_BINS") == nullptr) {
    const bool fresh = c->fine.p == nullptr;
    rc = ensure (c->fine, (size_t) BS_MAXBINS * 4, c->stream);
    if (rc) return rc;
    if (fresh || c->fine_dirty) HIPCHK (hipMemsetAsync (c->fine.p, 0, (size_t) BS_MAXBINS * 4, c->stream));
    if (!c->bins.p) { rc = ensure (c->bins, (size_t) (BS_MAXBINS + 1) * 4, c->stream); c->bins_zeroed = false; if (rc) return rc; }   // (clear_buckets_kernel writes the step's counts there)
    fine = (u32 *) c->fine.p;
    c->fine_dirty = true;
  }
  const auto aggregate = c->W == 1 ? aggregate1_kernel : c->W == 2 ? aggregate2_kernel : aggregate4_kernel;   // (named kernels: profiles cite them)
  hipLaunchKernelGGL (aggregate, dim3 (TJ_P), dim3 (AG_BLOCK), 0, c->stream, BK, (u64 *) c->ovf.p, c->k, remove_biased, (u64 *) c->kept.p, f.kept_cap, c->d_fin, plan_cap, d_plan, fine, fine_bin_bits (c->k));
  HIPCHK (hipGetLastError ());
  // counters, bucket sizes and the aggregation's own counts, in one copy; then the buckets are emptied (the aggregation
  // consumed them: leftover rounds reuse their fronts) together with the counts the next aggregation adds to
  // (with the ordering step planned ahead the copy waits until that has run: clear_buckets_kernel keeps what it zeroes)
  rc = f.plan_ahead ? TJAMD_OK : queue_counter_copies (c);
  if (!rc) rc = clear_buckets (c, f.plan_ahead);
  if (rc) return rc;
  if (f.plan_ahead) { rc = finalise_binned (c, 0, min_coverage, plan_cap, wait); if (rc) return rc; }   // (ends with a copy of the counts and a synchronisation, or an event)
  else HIPCHK (hipStreamSynchronize (c->stream));
  f.state = f.plan_ahead && !wait ? FIN_EVENT : FIN_ARRIVED;
  return TJAMD_OK;
}

static int finalise_collect (tjamd_counter *c, int *status)
{
  FinCarry &f = c->fin;
  if (f.state == FIN_SETTLED) { f.state = FIN_IDLE; return finalise_status (c, status, c->status); }
  if (f.state == FIN_EVENT) HIPCHK (hipEventSynchronize (c->ev_done));
  f.state = FIN_IDLE;
  int rc = TJAMD_OK;
  if (f.speculative) {
    rc = apply_counter_copies (c, f.plan_ahead);
    const long n = c->n_raw_known;
    c->n_raw_known = 0; c->raw_bound = 0; c->bucket_bound = 0; c->chunk_bound = TJ_P;      // (the buckets are empty again)
    if (rc) return rc;
    if (n == 0) return finalise_status (c, status, 1);                                      // reference: src/hopo_counter.c:345-349
    if (n >= (1l << 31)) return set_err (TJAMD_ERR_CAPACITY, "%ld raw records exceed the reference's int n_elem", n);
  }
  if (f.plan_ahead) {
    // what the aggregation's last workgroup read against what the kernel boundary behind it shows (the
    // last-workgroup pattern has no fence); a difference is repaired by sizing the ordering step again, from the exact count
    FinPlan &pl = c->h_state->plan;
    if (pl.n1 != pl.n1_exact || pl.kept_overflow != pl.ovf_exact) {
      c->plan_mismatches++;
      pl.n1 = pl.n1_exact; pl.kept_overflow = pl.ovf_exact; pl.ok = 0;
    }
  }
  if (f.plan_ahead ? c->h_state->plan.kept_overflow : c->h_fin->overflow) return set_err (TJAMD_ERR_CAPACITY, "kept list overflow");
  const long n1 = f.plan_ahead ? c->h_state->plan.n1 : (long) c->h_fin->n_kept;
  if (n1 == 0) {                                                               // reference :376-381
    rc = end_fin_interval (c, c->stream);
    return rc ? rc : finalise_status (c, status, 2);
  }

  // steps 3-4 + coverage: bin partition, then one pass per bin sorts it and derives the context index ranges and the
  // coverage table entries; the stable radix passes + separate index kernels take over if a bin is too full.
  c->n_kept = n1;
  if (!(f.plan_ahead && c->h_state->plan.ok)) rc = finalise_binned (c, n1, f.min_coverage);   // (not done yet, or more kept than planned for)
  if (!rc && c->h_fin->sort_fallback) rc = finalise_radix (c, n1, f.min_coverage);
  if (rc) return rc;
  c->n_idx = (int) c->h_fin->n_idx;
  if (c->n_idx == 0) return finalise_status (c, status, 3);   // reference :406-411 (coverage not estimated)
  c->coverage = c->h_fin->coverage;
  return finalise_status (c, status, 0);
}

extern "C" int tjamd_finalise (tjamd_counter *c, int remove_biased, int min_coverage, int *status)
{ const int rc = finalise_queue (c, remove_biased, min_coverage, true); return rc ? rc : finalise_collect (c, status); }
extern "C" int tjamd_finalise_begin (tjamd_counter *c, int remove_biased, int min_coverage) { return finalise_queue (c, remove_biased, min_coverage, false); }
extern "C" int tjamd_finalise_end (tjamd_counter *c, int *status)
{
  if (!c) return set_err (TJAMD_ERR_ARG, "null counter");
  if (c->fin.state == FIN_IDLE) return set_err (TJAMD_ERR_STATE, "tjamd_finalise_end without tjamd_finalise_begin");
  if (c->fin.state != FIN_SETTLED) HIPCHK (hipSetDevice (c->device));   // (settled: nothing is asked of the device)
  return finalise_collect (c, status);
}

extern "C" long tjamd_kept_count (tjamd_counter *c) { return c ? c->n_kept : -1; }
extern "C" int tjamd_n_idx (tjamd_counter *c) { return c ? c->n_idx : -1; }
extern "C" int tjamd_coverage (tjamd_counter *c) { return c ? c->coverage : -1; }
extern "C" const void *tjamd_kept_device_ptr (tjamd_counter *c) { return c ? c->kept.p : NULL; }

extern "C" long tjamd_download_kept (tjamd_counter *c, hopo_element *out, long capacity)
{
  if (!c) return -set_err (TJAMD_ERR_ARG, "null counter");
  if (c->status < 0) return -set_err (TJAMD_ERR_STATE, "counter not finalised");
  const long n1 = c->n_kept;
  if (n1 > capacity) return -set_err (TJAMD_ERR_CAPACITY, "%ld kept records, caller capacity %ld", n1, capacity);
  if (n1 == 0) return 0;
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  // (into pinned memory that the counter keeps: a fresh pageable vector of n1 records cost its page faults and a staged
  // copy every time -- a third of what finalise_hopo_counter spends behind the device finalise)
  if ((size_t) n1 * 24 > c->h_kept_cap) {
    if (c->h_kept) (void) hipHostFree (c->h_kept);
    c->h_kept = nullptr; c->h_kept_cap = 0;
    const size_t want = (size_t) n1 * 24 + ((size_t) n1 * 24 >> 2) + 4096;
    if (hipHostMalloc (&c->h_kept, want, hipHostMallocDefault) != hipSuccess) { c->h_kept = nullptr; return -set_err (TJAMD_ERR_HIP, "hipHostMalloc of %zu bytes failed", want); }
    c->h_kept_cap = want;
  }
  const tjamd_record *tmp = (const tjamd_record *) c->h_kept;
  if (hipMemcpyAsync (c->h_kept, c->kept.p, (size_t) n1 * 24, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize (c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "download failed");
  for (long i = 0; i < n1; i++) {
    out[i].context[0] = tmp[i].ctx0; out[i].context[1] = tmp[i].ctx1;
    memcpy ((char *) &out[i] + 16, &tmp[i].meta, 8);
    out[i].read_offset = -1;                    // state after reference src/hopo_counter.c:511
    out[i].loc_ref_id = out[i].loc_pos = out[i].loc_last = -1;
  }
  return n1;
}

extern "C" long tjamd_download_idx (tjamd_counter *c, int *idx_initial, int *idx_final, long capacity)
{
  if (!c) return -set_err (TJAMD_ERR_ARG, "null counter");
  if (c->status < 0) return -set_err (TJAMD_ERR_STATE, "counter not finalised");
  const long n = c->n_idx;
  if (n > capacity) return -set_err (TJAMD_ERR_CAPACITY, "%ld index ranges, caller capacity %ld", n, capacity);
  if (n == 0) return 0;
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  if (hipMemcpy (idx_initial, c->idx_i.p, (size_t) n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy (idx_final, c->idx_f.p, (size_t) n * 4, hipMemcpyDeviceToHost) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "download failed");
  return n;
}

extern "C" double tjamd_last_scan_ms (tjamd_counter *c)
{
  float ms = 0.f;
  if (!c || !c->timer[T_SCAN].elapsed (c->device, ms)) return -1.0;
  // (a stream scanned in pieces: the partition kernels between the scans are not the scan's time)
  for (int i = 0; i < c->n_piece_ev; i++) { float p = 0.f; if (hipEventElapsedTime (&p, c->ev_pa[i], c->ev_pb[i]) == hipSuccess) ms -= p; }
  return (double) ms;
}

// the kernels of the last tjamd_merge_samples on this counter (bin path), HIP events on its stream
TJ_LAST_MS (tjamd_last_merge_ms, T_MERGE)

// 1: one-word records go through the record log and partition_log_kernel (k <= 12, the default); 0: every scan kernel
// partitions its records itself
extern "C" int tjamd_counter_uses_log (const tjamd_counter *c) { return (c && c->W <= c->log_mode && c->fast_mode) ? 1 : 0; }

extern "C" double tjamd_last_partition_ms (tjamd_counter *c)
{ // partition_log_kernel behind the last scan launch (k <= 12, record log); 0 when the scan partitioned by itself
  if (!c || !c->timer[T_SCAN].timed) return -1.0;
  if (!c->part_timed) return 0.0;
  float ms = 0.f;
  if (hipSetDevice (c->device) != hipSuccess || hipEventSynchronize (c->ev_p1) != hipSuccess || hipEventElapsedTime (&ms, c->timer[T_SCAN].e1, c->ev_p1) != hipSuccess) return -1.0;
  for (int i = 0; i < c->n_piece_ev; i++) { float p = 0.f; if (hipEventElapsedTime (&p, c->ev_pa[i], c->ev_pb[i]) == hipSuccess) ms += p; }   // (the pieces before the last)
  return (double) ms;
}

TJ_LAST_MS (tjamd_last_finalise_ms, T_FIN)

extern "C" long tjamd_last_scan_launches (tjamd_counter *c) { return c ? c->last_scan_launches : -1; }
extern "C" long tjamd_plan_mismatches (tjamd_counter *c) { return c ? c->plan_mismatches : -1; }

// radix path of the merge: tag, stable sort, run heads, scans (any size, any skew)
static long merge_samples_radix (tjamd_counter *c, const void *d_records, long n, int n_samples, void *d_out_keys, void *d_out_counts, long capacity);

// ---------------------------------------------------------------------------------------------------------------
// "next" rows N3 / N1 on the device: grouping of near-identical contexts within a sample, tract ids on a union.
//
// Grouping (reference: new_genomic_context_list, src/context_histogram.c:245-270 with the distance of :25-48): the
// reference walks the elements in order and lets element i join the group being built iff it has the group's base and
// is closer than max_distance_per_flank (differing flank bases, both flanks together) to EVERY context already in it;
// otherwise i starts a new group.  (It walks them in BWA-location order and retries with a Levenshtein distance; here
// the order is the finalised array's own and there is no retry: the aligner and biomcmc-lib are absent.)
// On the device: back[i] = nearest j < i that element i could not share a group with (a thread walks back until it
// meets one); i can join iff the current group started after back[i].  Positions with back[i] == i - 1 start a group
// whatever came before, so the array falls into independent stretches, each walked by one thread.

__device__ __forceinline__ int flank_hamming (u64 a, u64 b)
{ // differing 2-bit positions of two packed k-mers (reference: src/hopo_counter.c:61-68 counts them one by one)
  const u64 d = a ^ b;
  return __popcll ((d | (d >> 1)) & 0x5555555555555555ull);
}

__global__ void group_back_kernel (const u64 *__restrict__ kept, long n, int maxd, int *__restrict__ back)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    const u64 c0 = kept[3 * i], c1 = kept[3 * i + 1], base = kept[3 * i + 2] & 3ull;
    long j = i - 1;
    while (j >= 0 && (kept[3 * j + 2] & 3ull) == base && flank_hamming (kept[3 * j], c0) + flank_hamming (kept[3 * j + 1], c1) < maxd) j--;
    back[i] = (int) j;
  }
}

__global__ void group_resolve_kernel (const int *__restrict__ back, long n, u32 *__restrict__ head)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    if (back[i] != (int) i - 1) continue;               // (i == 0: back = -1) only stretch starts walk
    head[i] = 1u;
    long start = i;
    for (long j = i + 1; j < n && back[j] != (int) j - 1; j++) {
      if (start > (long) back[j]) head[j] = 0u;
      else { head[j] = 1u; start = j; }
    }
  }
}

struct GroupOut { int first, n_elem, n_context, mode; long long integral; };

__global__ void group_summary_kernel (const u64 *__restrict__ kept, long n, const u32 *__restrict__ head, const u32 *__restrict__ gid_excl,
                                      int *__restrict__ group_of, GroupOut *__restrict__ groups)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    if (!head[i]) continue;
    const int g = (int) gid_excl[i];                     // groups before this head
    GroupOut o = {(int) i, 0, 0, (int) i, 0};
    int mode_count = 0;
    for (long j = i; j < n && (j == i || !head[j]); j++) {   // (reference: context_histogram_add_hopo_elem, src/context_histogram.c:181-222)
      const u64 m = kept[3 * j + 2];
      const int cnt = meta_count (m);
      if (j == i || kept[3 * j] != kept[3 * (j - 1)] || kept[3 * j + 1] != kept[3 * (j - 1) + 1]) o.n_context++;
      if (j == i || mode_count < cnt) { mode_count = cnt; o.mode = (int) j; }
      o.integral += cnt; o.n_elem++;
      group_of[j] = g;
    }
    groups[g] = o;
  }
}

// ---- the whole grouping step of new_genomic_context_list (reference: src/context_histogram.c:245-270): an element that
// fails the flank-distance test against the histogram being built is tried again with an edit distance between the two
// "left.B.right" names (:19-23, :255-261: joins if it is below opt.levenshtein_distance and marks the histogram `indel`),
// then every histogram gets its tract-length histogram (:278-286).
//
// The retry makes the step sequential in principle: whether element i joins depends on which element currently carries
// the histogram's name (the one with the highest count so far).  On the device it is speculated: (1) the grouping without
// the retry (group_back / group_resolve above) is computed in parallel; (2) every element that opens a group there is
// tested, in parallel, against the name the group before it ends up with -- which is what the sequential pass would test it
// against as long as no retry has succeeded since the last point where both agree; (3) where such a test succeeds (rare:
// unrelated contexts are a dozen edits apart) one thread replays the reference's loop from there until it opens a group at
// an element that opens one in (1) as well -- from that element on the two passes are in the same state again.
//
// The edit distance stands for biomcmc_levenshtein_distance (s1, n, s2, n, 1, 1, true) of biomcmc-lib, whose source is
// absent from the reference tree: unit-cost global edit distance (UNPINNED, see oracle/context_oracle.c).

__device__ __forceinline__ u32 name_symbol (u64 c0, u64 c1, u32 base, int k, int t)
{ // t-th character of generate_name_from_flanking_contexts (context, base, k, false) as a small integer ('.' = 4)
  if (t < k) return (u32) (c0 >> (2 * t)) & 3u;
  if (t == k + 1) return base;
  if (t < k + 3) return 4u;
  return (u32) (c1 >> (2 * (t - k - 3))) & 3u;
}

__device__ int name_edit_distance (const u64 *__restrict__ kept, long a, long b, int k, int free_end)
{
  const u64 a0 = kept[3 * a], a1 = kept[3 * a + 1], b0 = kept[3 * b], b1 = kept[3 * b + 1];
  const u32 ab = (u32) (kept[3 * a + 2] & 3ull), bb = (u32) (kept[3 * b + 2] & 3ull);
  const int n = 2 * k + 3;
  unsigned char row[2 * 32 + 4];
  for (int y = 0; y <= n; y++) row[y] = (unsigned char) y;
  int early = n;                                        // (free_end) a used up before b
  for (int x = 1; x <= n; x++) {
    const u32 sb = name_symbol (b0, b1, bb, k, x - 1);
    int diag = row[0];
    row[0] = (unsigned char) x;
    for (int y = 1; y <= n; y++) {
      const int up = row[y];
      int best = diag + (name_symbol (a0, a1, ab, k, y - 1) == sb ? 0 : 1);
      best = min (best, min ((int) row[y - 1], up) + 1);
      diag = up; row[y] = (unsigned char) best;
    }
    early = min (early, (int) row[n]);
  }
  int result = row[n];
  if (free_end) {                                       // the other reading of the absent function's last argument: one name may end early
    result = min (result, early);
    for (int y = 0; y <= n; y++) result = min (result, (int) row[y]);
  }
  return result;
}

// join types on the device: 0 opened its histogram, 1 joined within the flank distance and met its own context in the
// list, 5 joined within the flank distance and added a context, 2 taken in by the retry (always adds a context); the host
// sees type & 3
#define GJ_ADDS_CONTEXT(t) ((t) != 1)

// Where an element's count comes from, for the histogram's name (its element with the highest count, the first on a tie):
// the 20-bit field of the record within a sample; the exact total over the samples for the rows of a union
// (tjamd_union_tracts: the union key's field wraps).
struct MetaCount { __device__ __forceinline__ int operator() (const u64 *__restrict__ kept, long i) const { return meta_count (kept[3 * i + 2]); } };
struct TotalCount
{
  const long long *__restrict__ total;
  __device__ __forceinline__ long long operator() (const u64 *__restrict__, long i) const { return total[i]; }
};

// (2): elements that open a group in the grouping without the retry, tested against the name of the group before them
template <class CountOf>
__global__ void group_speculate_kernel (const u64 *__restrict__ kept, long n, int k, int lev, int free_end, const u32 *__restrict__ head,
                                        u32 *__restrict__ cand, int *__restrict__ jt, u32 *__restrict__ n_cand, CountOf count_of)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    u32 c = 0;
    // (without the retry every context of a histogram is within the flank distance of every other, the distance loop runs
    // through all of them, and an identical context -- the element before, in the sorted array -- is met)
    jt[i] = head[i] ? 0 : ((kept[3 * i] == kept[3 * (i - 1)] && kept[3 * i + 1] == kept[3 * (i - 1) + 1]) ? 1 : 5);
    if (head[i] && i > 0 && ((kept[3 * i + 2] ^ kept[3 * (i - 1) + 2]) & 3ull) == 0ull) {
      long ph = i - 1;
      while (!head[ph]) ph--;
      long mode = ph;
      auto mc = count_of (kept, ph);
      for (long j = ph + 1; j < i; j++) { const auto cj = count_of (kept, j); if (cj > mc) { mc = cj; mode = j; } }
      if (name_edit_distance (kept, mode, i, k, free_end) < lev) { c = 1u; atomicAdd (n_cand, 1u); }
    }
    cand[i] = c;
  }
}

// (3): one workgroup walks the candidates in order; thread 0 replays the reference's loop from each one that lies past
// the stretch the replay before it covered.  Once a histogram holds a context that came in through the retry its contexts
// are no longer all close to one another, and the reference's distance loop (src/context_histogram.c:36-46) matters as
// written: contexts in the order they were added, give up at the first one 2 * max_distance or more away, stop with
// distance 0 at an identical one (whatever comes after it), otherwise the largest distance met.
// lev_of (may be null): the edit distance that admitted each element taken in by the retry (type 2); other entries untouched.
#define GR_CHUNK 4096
template <class CountOf>
__global__ __launch_bounds__ (256)
void group_repair_kernel (const u64 *__restrict__ kept, long n, int k, int maxd, int lev, int free_end,
                          u32 *__restrict__ head, const u32 *__restrict__ cand, int *__restrict__ jt, CountOf count_of, int *__restrict__ lev_of)
{
  __shared__ long s_pos, s_min;
  if (threadIdx.x == 0) s_pos = 0;
  __syncthreads ();
  for (;;) {
    const long start = s_pos;
    if (start >= n) break;
    if (threadIdx.x == 0) s_min = n;
    __syncthreads ();
    const long end = min (n, start + (long) GR_CHUNK);
    for (long i = start + threadIdx.x; i < end; i += blockDim.x)
      if (cand[i]) { atomicMin ((unsigned long long *) &s_min, (unsigned long long) i); break; }
    __syncthreads ();
    const long h = s_min;
    if (threadIdx.x == 0) {
      if (h >= n) s_pos = end;
      else {
        long hd = h - 1;
        while (!head[hd]) hd--;                           // (flags before h are final: h lies past every earlier replay)
        long mode = hd;
        auto mc = count_of (kept, hd);
        for (long j = hd + 1; j < h; j++) { const auto cj = count_of (kept, j); if (cj > mc) { mc = cj; mode = j; } }
        long i = h;
        while (i < n) {
          if ((kept[3 * i + 2] ^ kept[3 * hd + 2]) & 3ull) break;          // another base: opens a group in both passes, untouched
          const u64 c0 = kept[3 * i], c1 = kept[3 * i + 1];
          int this_max = 0;
          bool fail = false, matched = false;
          for (long j = hd; j < i && !fail && !matched; j++) {
            if (j > hd && !GJ_ADDS_CONTEXT (jt[j])) continue;
            int d = min (flank_hamming (kept[3 * j], c0), 2 * maxd);
            if (d >= 2 * maxd) { fail = true; break; }
            d += min (flank_hamming (kept[3 * j + 1], c1), 2 * maxd - d);
            if (d >= 2 * maxd) { fail = true; break; }
            this_max = max (this_max, d);
            if (d == 0) matched = true;
          }
          int type = 0;
          if (!fail && (matched ? 0 : this_max) < maxd) type = matched ? 1 : 5;
          else {
            const int d = name_edit_distance (kept, mode, i, k, free_end);
            if (d < lev) { type = 2; if (lev_of) lev_of[i] = d; }       // the indel retry
          }
          if (type) {
            head[i] = 0u; jt[i] = type;
            const auto ci = count_of (kept, i);
            if (ci > mc) { mc = ci; mode = i; }
            i++;
          }
          else {
            const bool was_head = head[i] != 0u;
            head[i] = 1u; jt[i] = 0; hd = i; mode = i; mc = count_of (kept, i);
            i++;
            if (was_head) break;                          // both passes open a group here: the same state from now on
          }
        }
        s_pos = i;
      }
    }
    __syncthreads ();
  }
}

// The words behind the scan's own in c->scan_tmp: [0] receives the scan's total, [1] counts the candidates of the retry
static u32 *scan_total (tjamd_counter *c, long n) { return (u32 *) c->scan_tmp.p + scan_tmp_words (n); }

// scratch of queue_group_heads for n rows (retry: the retry's as well)
static int ensure_group_scratch (tjamd_counter *c, long n, bool retry)
{
  int rc = ensure (c->headpos, (size_t) n * 4, c->stream);          // back[]
  if (!rc) rc = ensure (c->flags, (size_t) n * 4, c->stream);      // head flags
  if (!rc) rc = ensure (c->outpos, (size_t) n * 4, c->stream);     // groups before each row
  if (!rc) rc = ensure (c->scan_tmp, scan_tmp_words (n) * 4 + 64, c->stream);
  if (retry && !rc) rc = ensure (c->keep, (size_t) n * 4, c->stream);       // candidates of the retry
  if (retry && !rc) rc = ensure (c->grp_jt, (size_t) n * 4, c->stream);     // join types
  return rc;
}

// Queues the grouping of the n rows of keys (tjamd_record[n] on the device) on the counter's stream, scratch from
// ensure_group_scratch.  It leaves the head flags (1 on the row that opens a group) in c->flags, the number of groups
// before each row in c->outpos and the number of groups in scan_total (c, n)[0]: on the device, the caller fetches it with
// its own results.  retry false: the flank test alone, nothing else is touched.  retry true: the edit-distance retry as
// well, a row's count coming from count_of; the join type of every row (GJ_ADDS_CONTEXT above, not yet & 3) is left in
// c->grp_jt, the distance that admitted each row of type 2 in lev_of, the number of candidates in *n_cand (either may be null);
// c->keep is used up.  Fetching that number is the one host round trip.  who: what the messages begin with.
template <class CountOf>
static int queue_group_heads (tjamd_counter *c, const char *who, const u64 *keys, long n, int maxd, CountOf count_of,
                              bool retry, int lev, int *lev_of, long *n_cand)
{
  u32 *head = (u32 *) c->flags.p, *total = scan_total (c, n), *d_cand = total + 1;
  hipLaunchKernelGGL (group_back_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, keys, n, maxd, (int *) c->headpos.p);
  hipLaunchKernelGGL (group_resolve_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const int *) c->headpos.p, n, head);
  if (retry) {
    if (hipMemsetAsync (d_cand, 0, 4, c->stream) != hipSuccess) return set_err (TJAMD_ERR_HIP, "memset failed");
    // (which reading of the absent edit distance's last argument: looked up per call -- tests switch it)
    const char *ed = getenv ("TATAJUBA_AMD_EDIT_DISTANCE");
    const int free_end = (ed && !strcmp (ed, "free_end")) ? 1 : 0;
    hipLaunchKernelGGL (group_speculate_kernel<CountOf>, dim3 (grid_for (n)), dim3 (256), 0, c->stream, keys, n, c->k, lev, free_end,
                        (const u32 *) head, (u32 *) c->keep.p, (int *) c->grp_jt.p, d_cand, count_of);
    if (hipGetLastError () != hipSuccess) return set_err (TJAMD_ERR_HIP, "%sgrouping launch failed", who);
    u32 nc = 0;
    if (hipMemcpyAsync (&nc, d_cand, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize (c->stream) != hipSuccess)
      return set_err (TJAMD_ERR_HIP, "%sgrouping failed: %s", who, hipGetErrorString (hipGetLastError ()));
    if (nc) hipLaunchKernelGGL (group_repair_kernel<CountOf>, dim3 (1), dim3 (256), 0, c->stream, keys, n, c->k, maxd, lev, free_end,
                                head, (const u32 *) c->keep.p, (int *) c->grp_jt.p, count_of, lev_of);
    if (n_cand) *n_cand = (long) nc;
  }
  return exclusive_scan (c, (const u32 *) head, (u32 *) c->outpos.p, n, total);
}

extern "C" long tjamd_group_contexts (tjamd_counter *c, int max_distance_per_flank, int *group_of, tjamd_group *groups, long capacity)
{
  if (!c || max_distance_per_flank < 0) return -set_err (TJAMD_ERR_ARG, "bad arguments");
  if (c->status < 0) return -set_err (TJAMD_ERR_STATE, "tjamd_group_contexts needs a finalised counter");
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  const long n = c->n_kept;
  if (n == 0) return 0;
  static_assert (sizeof (GroupOut) == sizeof (tjamd_group), "group layout");
  int rc = ensure_group_scratch (c, n, false);
  if (!rc) rc = ensure (c->segid, (size_t) n * 4, c->stream);      // group_of
  if (!rc) rc = ensure (c->alt, (size_t) n * sizeof (GroupOut), c->stream);
  if (rc) return -rc;
  const u64 *kept = (const u64 *) c->kept.p;
  rc = queue_group_heads (c, "", kept, n, max_distance_per_flank, MetaCount (), false, 0, nullptr, nullptr);   // the flank test alone
  if (rc) return -rc;
  hipLaunchKernelGGL (group_summary_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, kept, n, (const u32 *) c->flags.p, (const u32 *) c->outpos.p,
                      (int *) c->segid.p, (GroupOut *) c->alt.p);
  u32 ng = 0;
  rc = read_back (c, "tjamd_group_contexts", scan_total (c, n), &ng, 1);
  if (rc) return -rc;
  if ((long) ng > capacity && groups) return -set_err (TJAMD_ERR_CAPACITY, "%u groups, caller capacity %ld", ng, capacity);
  if (group_of && hipMemcpy (group_of, c->segid.p, (size_t) n * 4, hipMemcpyDeviceToHost) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "copy failed");
  if (groups && hipMemcpy (groups, c->alt.p, (size_t) ng * sizeof (GroupOut), hipMemcpyDeviceToHost) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "copy failed");
  return (long) ng;
}

struct CtxGroupOut { int first, n_elem, n_context, mode, indel, n_len, modal_len, modal_freq; long long integral; };
struct LenFreq { int length, freq; };

__global__ void group_histogram_kernel (const u64 *__restrict__ kept, long n, const u32 *__restrict__ head, const u32 *__restrict__ gid_excl,
                                        int *__restrict__ jt, int *__restrict__ group_of, CtxGroupOut *__restrict__ groups, LenFreq *__restrict__ hist)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    if (!head[i]) continue;
    const int g = (int) gid_excl[i];
    CtxGroupOut o = {(int) i, 0, 0, (int) i, 0, 0, 0, 0, 0};
    int mode_count = 0;
    LenFreq *h = hist + i;                              // (a histogram has at most as many lengths as its group has elements)
    for (long j = i; j < n && (j == i || !head[j]); j++) {
      const u64 m = kept[3 * j + 2];
      const int cnt = meta_count (m);
      const int len = meta_len (m);
      // contexts of the histogram (reference: context_histogram_add_hopo_elem, src/context_histogram.c:184-190): one more unless
      // the distance loop met an identical context; an element taken in by the indel retry is appended whatever the list holds
      const int t = jt[j];
      if (j == i || GJ_ADDS_CONTEXT (t)) o.n_context++;
      if (t == 2) o.indel = 1;
      jt[j] = t & 3;
      if (j == i || mode_count < cnt) { mode_count = cnt; o.mode = (int) j; }
      o.integral += cnt; o.n_elem++;
      int q = 0;
      while (q < o.n_len && h[q].length != len) q++;
      if (q == o.n_len) { h[q].length = len; h[q].freq = 0; o.n_len++; }
      h[q].freq += cnt;
      group_of[j] = g;
    }
    for (int a = 1; a < o.n_len; a++) {                 // highest summed count first, then the larger length (insertion sort: a few entries)
      const LenFreq x = h[a];
      int b = a - 1;
      while (b >= 0 && (h[b].freq < x.freq || (h[b].freq == x.freq && h[b].length < x.length))) { h[b + 1] = h[b]; b--; }
      h[b + 1] = x;
    }
    o.modal_len = h[0].length; o.modal_freq = h[0].freq;
    groups[g] = o;
  }
}

extern "C" long tjamd_context_histograms (tjamd_counter *c, int max_distance_per_flank, int levenshtein_distance, int *group_of, int *join_type,
                                          tjamd_context_group *groups, tjamd_length_freq *hist, long capacity)
{
  if (!c || max_distance_per_flank < 0) return -set_err (TJAMD_ERR_ARG, "bad arguments");
  if (c->status < 0) return -set_err (TJAMD_ERR_STATE, "tjamd_context_histograms needs a finalised counter");
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  const long n = c->n_kept;
  if (n == 0) return 0;
  static_assert (sizeof (CtxGroupOut) == sizeof (tjamd_context_group) && sizeof (LenFreq) == sizeof (tjamd_length_freq), "group layout");
  int rc = ensure_group_scratch (c, n, true);
  if (!rc) rc = ensure (c->segid, (size_t) n * 4, c->stream);      // group_of
  if (!rc) rc = ensure (c->grp_hist, (size_t) n * sizeof (LenFreq), c->stream);
  if (!rc) rc = ensure (c->alt, (size_t) n * sizeof (CtxGroupOut), c->stream);
  if (rc) return -rc;
  const u64 *kept = (const u64 *) c->kept.p;
  rc = queue_group_heads (c, "", kept, n, max_distance_per_flank, MetaCount (), true, levenshtein_distance, nullptr, nullptr);
  if (rc) return -rc;
  hipLaunchKernelGGL (group_histogram_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, kept, n, (const u32 *) c->flags.p, (const u32 *) c->outpos.p,
                      (int *) c->grp_jt.p, (int *) c->segid.p, (CtxGroupOut *) c->alt.p, (LenFreq *) c->grp_hist.p);
  u32 ng = 0;
  rc = read_back (c, "tjamd_context_histograms", scan_total (c, n), &ng, 1);
  if (rc) return -rc;
  if ((long) ng > capacity && groups) return -set_err (TJAMD_ERR_CAPACITY, "%u groups, caller capacity %ld", ng, capacity);
  if (group_of && hipMemcpy (group_of, c->segid.p, (size_t) n * 4, hipMemcpyDeviceToHost) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "copy failed");
  if (join_type && hipMemcpy (join_type, c->grp_jt.p, (size_t) n * 4, hipMemcpyDeviceToHost) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "copy failed");
  if (groups && hipMemcpy (groups, c->alt.p, (size_t) ng * sizeof (CtxGroupOut), hipMemcpyDeviceToHost) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "copy failed");
  if (hist && hipMemcpy (hist, c->grp_hist.p, (size_t) n * sizeof (LenFreq), hipMemcpyDeviceToHost) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "copy failed");
  return (long) ng;
}

// Tract ids on a merged union (reference: src/genome_set.c:207-221: the id goes up wherever two neighbours of the
// concatenated list do not overlap; context-keyed: wherever (base, ctx0, ctx1) changes).  d_keys: tjamd_record[n] in the
// reference's descending order, as tjamd_merge_samples writes them.
__global__ void tract_head_kernel (const u64 *__restrict__ keys, long n, u32 *__restrict__ head)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x)
    head[i] = (i > 0 && !same_context_rows (keys, i, i - 1)) ? 1u : 0u;
}
__global__ void tract_id_kernel (const u32 *__restrict__ excl, const u32 *__restrict__ head, long n, int *__restrict__ id)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) id[i] = (int) (excl[i] + head[i]);
}

static int ensure_tract_id_scratch (tjamd_counter *c, long n)
{
  int rc = ensure (c->flags, (size_t) n * 4, c->stream);
  if (!rc) rc = ensure (c->outpos, (size_t) n * 4, c->stream);
  if (!rc) rc = ensure (c->segid, (size_t) n * 4, c->stream);
  if (!rc) rc = ensure (c->scan_tmp, scan_tmp_words (n) * 4 + 64, c->stream);
  return rc;
}

// queues the id pass on the counter's stream (scratch from ensure_tract_id_scratch); the number of heads lands in *total
static int queue_tract_ids (tjamd_counter *c, const void *d_keys, long n, int *ids, u32 *total)
{
  hipLaunchKernelGGL (tract_head_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const u64 *) d_keys, n, (u32 *) c->flags.p);
  int rc = exclusive_scan (c, (const u32 *) c->flags.p, (u32 *) c->outpos.p, n, total);
  if (rc) return rc;
  hipLaunchKernelGGL (tract_id_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const u32 *) c->outpos.p, (const u32 *) c->flags.p, n, ids);
  if (hipGetLastError () != hipSuccess) return set_err (TJAMD_ERR_HIP, "tract id launch failed");
  return TJAMD_OK;
}

extern "C" long tjamd_tract_ids (tjamd_counter *c, const void *d_keys, long n, int *d_tract_id, int *h_tract_id)
{
  if (!c || n < 0 || (n && !d_keys)) return -set_err (TJAMD_ERR_ARG, "bad arguments");
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  if (n == 0) return 0;
  int rc = ensure_tract_id_scratch (c, n);
  if (rc) return -rc;
  u32 *total = scan_total (c, n);
  int *ids = d_tract_id ? d_tract_id : (int *) c->segid.p;
  rc = queue_tract_ids (c, d_keys, n, ids, total);
  if (rc) return -rc;
  u32 nh = 0;
  rc = read_back (c, "tjamd_tract_ids", total, &nh, 1);
  if (rc) return -rc;
  if (h_tract_id && hipMemcpy (h_tract_id, ids, (size_t) n * 4, hipMemcpyDeviceToHost) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "copy failed");
  return (long) nh + 1;
}

// ---------------------------------------------------------------------------------------------------------------
// Per-tract statistics across samples and the variable tracts (reference: describe_statistics_for_genome_set,
// src/genome_set.c:619-678; descriptive_stats_of_histogram :738-766; relative_difference_of_vector :768-779;
// update_descriptive_stats_for_this_trait :692-710).  One segment of S = min (64, next_pow2 (n_samples)) lanes per tract,
// 64 / S tracts per wavefront: a lane takes samples lane, lane + S, ..., so a count row is read as S contiguous words;
// the min / max / presence over the samples are reduced across the segment with shuffles.  No atomics on values.

struct TractSummary { int first, n_rows, n_present, variable; double reldiff[TJAMD_N_TRACT_STATS]; };
static_assert (sizeof (TractSummary) == 56 && sizeof (TractSummary) == sizeof (tjamd_tract_summary), "tract summary layout");

// tract starts from the ids: first row at the head, one past the last row (n_rows is made of it by tract_stats_kernel) at
// the tail; err[0] |= 1 where the ids do not start at 0 or go up by something other than 0 or 1 (nothing is written then
// outside [0, cap)); err[1] = the last row's id
__global__ void tract_starts_kernel (const int *__restrict__ id, long n, long cap, TractSummary *__restrict__ sum, int *__restrict__ err)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    const int a = id[i];
    const long step = i ? (long) a - (long) id[i - 1] : (a == 0 ? 1l : -1l);   // (row 0: id 0 and nothing else)
    if (step != 0 && step != 1) { atomicOr (err, 1); continue; }
    if (i == n - 1) err[1] = a;
    if (a < 0 || a >= cap) continue;                    // (after a bad step elsewhere; or more tracts than the caller has room for)
    if (step == 1) sum[a].first = (int) i;
    if (i == n - 1 || id[i + 1] != a) sum[a].n_rows = (int) (i + 1);
  }
}

// the five values of one (tract, sample) (descriptive_stats_of_histogram), its modal length and n_context; false if absent
__device__ bool tract_sample_values (const u64 *__restrict__ keys, const int *__restrict__ counts, int ns, long first, long end, int s, int cov,
                                     double *v, int &modal_len, int &n_ctx)
{
  long long integral = 0;
  int maxc = 0, modal = 0, nctx = 0;
  long prev = -1;
  for (long r = first; r < end; r++) {
    const int cnt = counts[r * ns + s];
    if (cnt == 0) continue;
    const int len = meta_len (keys[3 * r + 2]);
    if (prev < 0 || !same_context_rows (keys, r, prev)) nctx++;
    if (prev < 0 || cnt > maxc || (cnt == maxc && len > modal)) { maxc = cnt; modal = len; }
    integral += cnt;
    prev = r;
  }
  modal_len = 0; n_ctx = 0;
  for (int j = 0; j < TJAMD_N_TRACT_STATS; j++) v[j] = 0.0;
  if (prev < 0) return false;
  const double I = (double) integral;
  double avg = 0.0, ent = 0.0;
  for (long r = first; r <= prev; r++) {                // the reference's sums, bar by bar (:746-747, :758-761)
    const int cnt = counts[r * ns + s];
    if (cnt == 0) continue;
    const int len = meta_len (keys[3 * r + 2]);
    avg += (double) ((long long) cnt * len) / I;
    const double x = (double) cnt / I;
    ent += x * log (x);
  }
  v[TJAMD_STAT_AVG_LENGTH] = avg;
  v[TJAMD_STAT_MODAL_FREQ] = (double) maxc / I;
  v[TJAMD_STAT_PROP_COVERAGE] = I / (double) cov;
  v[TJAMD_STAT_COVERAGE_PER_CONTEXT] = I / (double) nctx;
  v[TJAMD_STAT_ENTROPY] = -ent;
  modal_len = modal; n_ctx = nctx;
  return true;
}

__device__ __forceinline__ double dmax_ref (double a, double b) { return (a < b) ? b : a; }   // relative_difference_of_vector's comparisons
__device__ __forceinline__ double dmin_ref (double a, double b) { return (a > b) ? b : a; }

// What a segment of S lanes gathers about one tract, a lane taking samples lane, lane + S, ...: the largest and smallest of
// each of the five values over the samples that have the tract, how many have it, whether one's modal length is off the
// reference's (ref > 0).  Both statistics kernels fill it; how a sample's five values are computed is theirs.
struct TractSpread
{
  double mx[TJAMD_N_TRACT_STATS], mn[TJAMD_N_TRACT_STATS];
  int present = 0, off_ref = 0;
  __device__ __forceinline__ TractSpread () { for (int j = 0; j < TJAMD_N_TRACT_STATS; j++) { mx[j] = -FLT_MAX; mn[j] = FLT_MAX; } }
  __device__ __forceinline__ void add (const double *v, int modal_len, int ref)
  { // one sample that has the tract
    present++;
    if (ref > 0 && modal_len != ref) off_ref = 1;
    for (int j = 0; j < TJAMD_N_TRACT_STATS; j++) { mx[j] = dmax_ref (mx[j], v[j]); mn[j] = dmin_ref (mn[j], v[j]); }
  }
  __device__ __forceinline__ void reduce (int S)
  { // over the segment: every lane ends with the whole
    for (int o = 1; o < S; o <<= 1) {
      present += __shfl_xor (present, o, S);
      off_ref |= __shfl_xor (off_ref, o, S);
      for (int j = 0; j < TJAMD_N_TRACT_STATS; j++) {
        mx[j] = dmax_ref (mx[j], __shfl_xor (mx[j], o, S));
        mn[j] = dmin_ref (mn[j], __shfl_xor (mn[j], o, S));
      }
    }
  }
  __device__ __forceinline__ int finish (int ns, double *reldiff) const
  { // relative_difference_of_vector per value; returns whether the tract is variable (update_descriptive_stats_for_this_trait)
    for (int j = 0; j < TJAMD_N_TRACT_STATS; j++) reldiff[j] = (mx[j] > DBL_MIN) ? mx[j] - mn[j] : 0.0;
    const double difference = reldiff[TJAMD_STAT_AVG_LENGTH] + reldiff[TJAMD_STAT_MODAL_FREQ] + reldiff[TJAMD_STAT_ENTROPY];
    return (present < ns || difference > 1.e-5 || off_ref) ? 1 : 0;
  }
};

// An entry of a caller's list of tracts against the summaries it names (TractSummary, UnionSummary: both begin with first,
// n_rows): the tract's rows; no rows and err |= 1 where the id is outside [0, n_tracts) or the rows outside the union.
template <class Summary>
__device__ __forceinline__ void listed_tract_rows (const Summary *sum, long n_tracts, long n_union, int t, int lane, int *err, long &first, long &end)
{
  first = 0; end = 0;
  if (t >= 0 && t < n_tracts) { first = sum[t].first; end = first + (long) sum[t].n_rows; }
  const bool ok = t >= 0 && t < n_tracts && first >= 0 && first <= end && end <= n_union;
  if (!ok) { if (lane == 0) atomicOr (err, 1); first = end = 0; }
}

// sample s of list entry i: its five values, modal length and n_context (the last two may be null)
__device__ __forceinline__ void write_listed_sample (long i, int s, int ns, const double *v, int ml, int nc,
                                                     double *__restrict__ values, int *__restrict__ modal_len, int *__restrict__ n_context)
{
  for (int j = 0; j < TJAMD_N_TRACT_STATS; j++) values[(i * TJAMD_N_TRACT_STATS + j) * ns + s] = v[j];
  if (modal_len) modal_len[i * ns + s] = ml;
  if (n_context) n_context[i * ns + s] = nc;
}

// The segment mapping of the kernels that give an item (a tract, a list entry, a row) S lanes, S a power of two that divides the
// workgroup: declares the thread's lane in its segment, its segment's first item and the stride to the next (the grid's segments).
// A macro: inside a function the compiler reads blockDim the long way, and every kernel that called one came out longer.
#define SEGMENT_MAP(S, lane, first, stride) \
  const int lane = threadIdx.x & ((S) - 1); \
  const long stride = (long) gridDim.x * (blockDim.x / (S)); \
  const long first = (blockIdx.x * (long) blockDim.x + threadIdx.x) / (S);

__global__ __launch_bounds__ (256)
void tract_stats_kernel (const u64 *__restrict__ keys, const int *__restrict__ counts, long n_union, int ns, int S, const int *__restrict__ cov,
                         const int *__restrict__ ref_len, TractSummary *__restrict__ sum, long n_bound, int *__restrict__ err, u32 *__restrict__ varflag)
{ // n_bound: the tracts the caller has room for; the tracts there are (err[1] + 1) and whether the ids were good (err[0] == 0)
  // come from tract_starts_kernel.  Every flag below n_bound is written (0 outside the tracts), so the scan behind is sound.
  // err[2]: set here if a tract's rows lie outside the union.
  const int lane = threadIdx.x & (S - 1);                // (SEGMENT_MAP written out: the load of n_tracts stands before the division)
  const long segs_per_grid = (long) gridDim.x * (blockDim.x / S);
  const long n_tracts = err[0] ? 0 : min ((long) err[1] + 1, n_bound);
  for (long t = (blockIdx.x * (long) blockDim.x + threadIdx.x) / S; t < n_bound; t += segs_per_grid) {   // (uniform across a segment)
    long first = 0, end = 0;                            // (tract_starts_kernel left one past the last row in n_rows)
    if (t < n_tracts) { first = sum[t].first; end = sum[t].n_rows; }
    if (t >= n_tracts || first < 0 || first >= end || end > n_union) {
      if (lane == 0) { varflag[t] = 0u; if (t < n_tracts) atomicOr (err + 2, 1); }   // (rows outside the union: cannot happen after good ids)
      continue;
    }
    const int ref = ref_len ? ref_len[t] : 0;
    TractSpread sp;
    for (int s = lane; s < ns; s += S) {
      double v[TJAMD_N_TRACT_STATS];
      int ml, nc;
      if (tract_sample_values (keys, counts, ns, first, end, s, cov[s], v, ml, nc)) sp.add (v, ml, ref);
    }
    sp.reduce (S);
    if (lane == 0) {
      TractSummary o;
      o.first = (int) first; o.n_rows = (int) (end - first); o.n_present = sp.present;
      o.variable = sp.finish (ns, o.reldiff);
      sum[t] = o;
      varflag[t] = (u32) o.variable;
    }
  }
}

__global__ void tract_var_scatter_kernel (const u32 *__restrict__ flag, const u32 *__restrict__ pos, long n, int *__restrict__ var)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x)
    if (flag[i]) var[pos[i]] = (int) i;
}

__global__ __launch_bounds__ (256)
void tract_sample_stats_kernel (const u64 *__restrict__ keys, const int *__restrict__ counts, long n_union, int ns, int S, const int *__restrict__ cov,
                                const TractSummary *__restrict__ sum, long n_tracts, const int *__restrict__ list, long n_list,
                                double *__restrict__ values, int *__restrict__ modal_len, int *__restrict__ n_context, int *__restrict__ err)
{
  SEGMENT_MAP (S, lane, first_item, segs_per_grid)
  for (long i = first_item; i < n_list; i += segs_per_grid) {
    long first, end;
    listed_tract_rows (sum, n_tracts, n_union, list[i], lane, err, first, end);
    for (int s = lane; s < ns; s += S) {
      double v[TJAMD_N_TRACT_STATS];
      int ml, nc;
      tract_sample_values (keys, counts, ns, first, end, s, cov[s], v, ml, nc);
      write_listed_sample (i, s, ns, v, ml, nc, values, modal_len, n_context);
    }
  }
}

static int tract_segment (int n_samples) { int S = 1; while (S < n_samples && S < 64) S <<= 1; return S; }
static unsigned tract_grid (long n, int S) { return (unsigned) std::max<long> (1, std::min<long> ((n * S + 255) / 256, 65536)); }

static int union_args (const char *fn, const void *d_keys, const void *d_counts, long n_union, int n_samples)
{ // the checks every entry that takes a union shares, before any device call
  if (n_union < 0) return set_err (TJAMD_ERR_ARG, "%s: n_union %ld < 0", fn, n_union);
  if (n_union >= (1l << 31)) return set_err (TJAMD_ERR_CAPACITY, "%s: %ld union rows", fn, n_union);
  if (n_samples < 1 || n_samples > 4096) return set_err (TJAMD_ERR_ARG, "%s: n_samples %d outside 1..4096", fn, n_samples);
  if (n_union > 0 && (!d_keys || !d_counts)) return set_err (TJAMD_ERR_ARG, "%s: null union buffers", fn);
  return TJAMD_OK;
}

static int tract_count_arg (const char *fn, long n_tracts, long n_union)
{ // tracts that tile a union: one at least unless it is empty, one per row at most
  return (n_tracts < (n_union > 0 ? 1 : 0) || n_tracts > n_union) ? set_err (TJAMD_ERR_ARG, "%s: n_tracts %ld for a union of %ld rows", fn, n_tracts, n_union) : TJAMD_OK;
}
static int tiled_union_args (const char *fn, const void *d_keys, const void *d_counts, long n_union, int n_samples, const void *d_tracts, long n_tracts, const void *d_tract_loc)
{ // ... a union, the tracts that tile it and a location per tract (N8, N13)
  int rc = union_args (fn, d_keys, d_counts, n_union, n_samples);
  if (!rc) rc = tract_count_arg (fn, n_tracts, n_union);
  if (!rc && n_tracts > 0 && (!d_tracts || !d_tract_loc)) rc = set_err (TJAMD_ERR_ARG, "%s: null tract or tract location buffer", fn);
  return rc;
}
// the refusal after the device found the tiling broken (tjamd_union_tract_stats words its own, which its callers match on)
static const char TILING_REFUSED[] = "%s: the tracts do not tile the union (first 0, each starting where the one before ends, the last ending at n_union)";

static int tract_args (const char *fn, const void *d_keys, const void *d_counts, long n_union, int n_samples, const int *coverage)
{ // ... and, for the statistics, the samples' coverages
  const int rc = union_args (fn, d_keys, d_counts, n_union, n_samples);
  if (rc) return rc;
  if (!coverage) return set_err (TJAMD_ERR_ARG, "%s: null coverage", fn);
  return TJAMD_OK;
}

static int upload_coverage (tjamd_counter *c, const int *coverage, int n_samples)
{
  int rc = ensure (c->ts_cov, (size_t) n_samples * 4, c->stream);
  if (!rc) rc = ensure (c->ts_aux, 64, c->stream);
  if (rc) return rc;
  HIPCHK (hipMemcpyAsync (c->ts_cov.p, coverage, (size_t) n_samples * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK (hipMemsetAsync (c->ts_aux.p, 0, 64, c->stream));
  return TJAMD_OK;
}

extern "C" long tjamd_tract_stats (tjamd_counter *c, const void *d_keys, const void *d_counts, long n_union, int n_samples,
                                   const int *d_tract_id, const int *coverage, const int *d_ref_length,
                                   tjamd_tract_summary *d_summary, int *d_var, long capacity, long *n_var)
{
  if (n_union > 0 && !d_summary) return -set_err (TJAMD_ERR_ARG, "tjamd_tract_stats: null summary buffer");
  if (capacity < (n_union > 0 ? 1 : 0)) return -set_err (TJAMD_ERR_CAPACITY, "tjamd_tract_stats: capacity %ld for a union of %ld rows", capacity, n_union);
  int rc = tract_args ("tjamd_tract_stats", d_keys, d_counts, n_union, n_samples, coverage);
  if (rc) return -rc;
  if (!c) return -set_err (TJAMD_ERR_ARG, "tjamd_tract_stats: null counter");
  if (n_var) *n_var = 0;
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  if (n_union == 0) return 0;
  // (no host round trip before the end: the kernels read the tract count and the id check from the device, and work on
  // n_bound tracts at most; a count above the caller's capacity is reported at the end, nothing having been written past it)
  const long n_bound = std::min (n_union, capacity);
  rc = ensure_tract_id_scratch (c, n_union);
  if (!rc) rc = upload_coverage (c, coverage, n_samples);
  if (rc) return -rc;
  Stage st (c, T_TRACT);
  st.begin ();
  u32 *total = scan_total (c, n_union);
  const int *ids = d_tract_id;
  if (!ids) {                                           // the context-keyed ids of tjamd_tract_ids, in c->segid
    rc = queue_tract_ids (c, d_keys, n_union, (int *) c->segid.p, total);
    if (rc) return -rc;
    ids = (const int *) c->segid.p;
  }
  int *err = (int *) c->ts_aux.p;
  hipLaunchKernelGGL (tract_starts_kernel, dim3 (grid_for (n_union)), dim3 (256), 0, c->stream, ids, n_union, n_bound, (TractSummary *) d_summary, err);
  const int S = tract_segment (n_samples);
  hipLaunchKernelGGL (tract_stats_kernel, dim3 (tract_grid (n_bound, S)), dim3 (256), 0, c->stream, (const u64 *) d_keys, (const int *) d_counts, n_union,
                      n_samples, S, (const int *) c->ts_cov.p, d_ref_length, (TractSummary *) d_summary, n_bound, err, (u32 *) c->flags.p);
  if (hipGetLastError () != hipSuccess) return -set_err (TJAMD_ERR_HIP, "tract stats launch failed");
  rc = exclusive_scan (c, (const u32 *) c->flags.p, (u32 *) c->outpos.p, n_bound, total);
  if (rc) return -rc;
  if (d_var) hipLaunchKernelGGL (tract_var_scatter_kernel, dim3 (grid_for (n_bound)), dim3 (256), 0, c->stream, (const u32 *) c->flags.p, (const u32 *) c->outpos.p,
                                 n_bound, d_var);
  if (hipGetLastError () != hipSuccess) return -set_err (TJAMD_ERR_HIP, "tract list launch failed");
  st.end ();
  int h_err[3] = {0, 0, 0};
  u32 nv = 0;
  if (hipMemcpyAsync (h_err, err, 12, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipMemcpyAsync (&nv, total, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize (c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "tract stats failed: %s", hipGetErrorString (hipGetLastError ()));
  const long n_tracts = (long) h_err[1] + 1;
  if (h_err[0] || h_err[2] || n_tracts < 1) return -set_err (TJAMD_ERR_ARG, "tjamd_tract_stats: tract ids must start at 0 and go up by 0 or 1 per row");
  if (n_tracts > capacity) return -set_err (TJAMD_ERR_CAPACITY, "tjamd_tract_stats: %ld tracts, caller capacity %ld", n_tracts, capacity);
  st.done ();
  if (n_var) *n_var = (long) nv;
  return n_tracts;
}

extern "C" long tjamd_tract_sample_stats (tjamd_counter *c, const void *d_keys, const void *d_counts, long n_union, int n_samples,
                                          const int *coverage, const tjamd_tract_summary *d_summary, long n_tracts, const int *d_list, long n_list,
                                          double *d_values, int *d_modal_len, int *d_n_context)
{
  int rc = tract_args ("tjamd_tract_sample_stats", d_keys, d_counts, n_union, n_samples, coverage);
  if (rc) return -rc;
  if (n_list < 0 || n_tracts < 0 || n_tracts > n_union) return -set_err (TJAMD_ERR_ARG, "tjamd_tract_sample_stats: n_list %ld, n_tracts %ld (union of %ld rows)", n_list, n_tracts, n_union);
  if (n_list > 0 && (!d_summary || !d_list || !d_values)) return -set_err (TJAMD_ERR_ARG, "tjamd_tract_sample_stats: null summary, list or values buffer");
  if (!c) return -set_err (TJAMD_ERR_ARG, "tjamd_tract_sample_stats: null counter");
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  if (n_list == 0) return 0;
  rc = upload_coverage (c, coverage, n_samples);
  if (rc) return -rc;
  const int S = tract_segment (n_samples);
  int *err = (int *) c->ts_aux.p, h_err = 0;
  hipLaunchKernelGGL (tract_sample_stats_kernel, dim3 (tract_grid (n_list, S)), dim3 (256), 0, c->stream, (const u64 *) d_keys, (const int *) d_counts, n_union,
                      n_samples, S, (const int *) c->ts_cov.p, (const TractSummary *) d_summary, n_tracts, d_list, n_list, d_values, d_modal_len, d_n_context, err);
  rc = read_back (c, "tjamd_tract_sample_stats", err, &h_err, 1);
  if (rc) return -rc;
  if (h_err) return -set_err (TJAMD_ERR_ARG, "tjamd_tract_sample_stats: a listed tract id is outside [0, %ld) or its rows outside the union", n_tracts);
  return n_list;
}

TJ_LAST_MS (tjamd_last_tract_stats_ms, T_TRACT)

// ---------------------------------------------------------------------------------------------------------------
// N6: tracts across samples by grouping (reference: new_genomic_context_list's grouping, src/context_histogram.c:245-270,
// taken as the cross-sample tract of new_g_tract_vector_from_genomic_context_list, src/genome_set.c:195-229; statistics
// of update_g_tract_summary_from_context_histogram / fill_g_tract_summary_tables :291-378; selection of
// print_selected_g_tract_vector :380-434).  The union rows are grouped as one pooled sample's finalised array would be
// (the N3 kernels above), a row's count being its exact total over the samples; a sample's histogram in a tract is then its
// non-zero rows summed per length, bars ordered by count (highest first), then length (larger first): the reference's h.

struct UnionTract { int first, n_rows, n_context, mode, indel, lev_distance; long long integral; };
static_assert (sizeof (UnionTract) == 32 && sizeof (UnionTract) == sizeof (tjamd_union_tract), "union tract layout");
struct UnionSummary { int first, n_rows, n_present, variable, selected, lev_distance; double reldiff[TJAMD_N_TRACT_STATS]; };
static_assert (sizeof (UnionSummary) == 64 && sizeof (UnionSummary) == sizeof (tjamd_union_tract_summary), "union summary layout");

// The tracts a caller passes (statistics, located tracts, N8, N9, N13) must tile the union: the first at row 0, each starting
// where the one before ends, the last ending at n_union.  tract_rows: a tract's rows [first, end), none where they do not lie
// inside the union, which keeps a refused call from reading outside it; breaks_tiling: whether tract t does; check_tiling: the
// whole grid, a thread per tract, err |= 1 where one does.
__device__ __forceinline__ void tract_rows (const UnionTract &u, long n_union, long &first, long &end)
{
  first = u.first; end = first + (long) u.n_rows;
  if (first < 0 || u.n_rows < 1 || end > n_union) first = end = 0;
}
__device__ __forceinline__ bool breaks_tiling (const UnionTract *__restrict__ tracts, long n_tracts, long n_union, long t)
{
  long first, end;
  tract_rows (tracts[t], n_union, first, end);
  const long want = t ? (long) tracts[t - 1].first + (long) tracts[t - 1].n_rows : 0l;
  return first == end || first != want || (t == n_tracts - 1 && end != n_union);
}
__device__ __forceinline__ void check_tiling (const UnionTract *__restrict__ tracts, long n_tracts, long n_union, int *__restrict__ err)
{
  for (long t = blockIdx.x * (long) blockDim.x + threadIdx.x; t < n_tracts; t += (long) gridDim.x * blockDim.x)
    if (breaks_tiling (tracts, n_tracts, n_union, t)) atomicOr (err, 1);
}
// a 64-bit word from lane `from` / from lane ^ o of a segment of `width` lanes
__device__ __forceinline__ u64 shfl64 (u64 x, int from, int width = 64) { const u32 lo = __shfl ((u32) x, from, width), hi = __shfl ((u32) (x >> 32), from, width); return ((u64) hi << 32) | lo; }
__device__ __forceinline__ u64 readlane64 (u64 x, int from) { return ((u64) (u32) __builtin_amdgcn_readlane ((int) (x >> 32), from) << 32) | (u32) __builtin_amdgcn_readlane ((int) x, from); }
__device__ __forceinline__ u64 shfl_xor64 (u64 x, int o, int width = 64) { const u32 lo = __shfl_xor ((u32) x, o, width), hi = __shfl_xor ((u32) (x >> 32), o, width); return ((u64) hi << 32) | lo; }

// exact row totals: one segment of S lanes per row, a lane summing samples lane, lane + S, ... (S contiguous words per step)
__global__ __launch_bounds__ (256)
void union_totals_kernel (const int *__restrict__ counts, long n, int ns, int S, long long *__restrict__ total)
{
  SEGMENT_MAP (S, lane, first_item, segs_per_grid)
  for (long r = first_item; r < n; r += segs_per_grid) {   // (uniform across a segment)
    long long t = 0;
    for (int s = lane; s < ns; s += S) t += counts[r * ns + s];
    for (int o = 1; o < S; o <<= 1) t += __shfl_xor (t, o, S);
    if (lane == 0) total[r] = t;
  }
}

// one thread per tract (at its head): the fields of tjamd_union_tract, the ids of its rows, their join types (type & 3)
__global__ void union_tract_kernel (long n, const long long *__restrict__ total, const u32 *__restrict__ head, const u32 *__restrict__ gid_excl,
                                    const int *__restrict__ jt, const int *__restrict__ lev_of, long cap, int *__restrict__ tract_id,
                                    int *__restrict__ join_type, UnionTract *__restrict__ tracts)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    if (!head[i]) continue;
    const int g = (int) gid_excl[i];
    UnionTract o = {(int) i, 0, 0, (int) i, 0, 0, 0};
    long long mode_count = 0;
    for (long j = i; j < n && (j == i || !head[j]); j++) {
      const int t = jt[j];
      if (j == i || GJ_ADDS_CONTEXT (t)) o.n_context++;   // (the rule of group_histogram_kernel)
      if (t == 2) { o.indel = 1; o.lev_distance = max (o.lev_distance, lev_of[j]); }   // (lev_of: written by the repair for every type 2)
      const long long cj = total[j];
      if (j == i || mode_count < cj) { mode_count = cj; o.mode = (int) j; }
      o.integral += cj; o.n_rows++;
      tract_id[j] = g;
      if (join_type) join_type[j] = t & 3;
    }
    if (g < cap) tracts[g] = o;
  }
}

extern "C" long tjamd_union_tracts (tjamd_counter *c, const void *d_keys, const void *d_counts, long n_union, int n_samples,
                                    int max_distance_per_flank, int levenshtein_distance,
                                    int *d_tract_id, int *d_join_type, tjamd_union_tract *d_tracts, long capacity)
{
  static const char *fn = "tjamd_union_tracts";
  int rc = union_args (fn, d_keys, d_counts, n_union, n_samples);
  if (rc) return -rc;
  if (n_union > 0 && (!d_tract_id || !d_tracts)) return -set_err (TJAMD_ERR_ARG, "%s: null tract id or tract buffer", fn);
  if (max_distance_per_flank < 0 || levenshtein_distance < 0)
    return -set_err (TJAMD_ERR_ARG, "%s: negative distance (max_distance_per_flank %d, levenshtein_distance %d)", fn, max_distance_per_flank, levenshtein_distance);
  if (capacity < (n_union > 0 ? 1 : 0)) return -set_err (TJAMD_ERR_CAPACITY, "%s: capacity %ld for a union of %ld rows", fn, capacity, n_union);
  if (!c) return -set_err (TJAMD_ERR_ARG, "%s: null counter", fn);
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  Stage st (c, T_UNION);
  c->union_cand = -1;
  const long n = n_union;
  if (n == 0) return 0;
  rc = ensure_group_scratch (c, n, true);
  if (!rc) rc = ensure (c->ut_tot, (size_t) n * 8, c->stream);
  if (!rc) rc = ensure (c->ut_lev, (size_t) n * 4, c->stream);
  if (rc) return -rc;
  long long *tot = (long long *) c->ut_tot.p;
  st.begin ();
  const int S = tract_segment (n_samples);
  hipLaunchKernelGGL (union_totals_kernel, dim3 (tract_grid (n, S)), dim3 (256), 0, c->stream, (const int *) d_counts, n, n_samples, S, tot);
  long n_cand = 0;
  rc = queue_group_heads (c, "tjamd_union_tracts: ", (const u64 *) d_keys, n, max_distance_per_flank, TotalCount {tot}, true, levenshtein_distance,
                          (int *) c->ut_lev.p, &n_cand);
  if (rc) return -rc;
  hipLaunchKernelGGL (union_tract_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, n, (const long long *) tot, (const u32 *) c->flags.p,
                      (const u32 *) c->outpos.p, (const int *) c->grp_jt.p, (const int *) c->ut_lev.p, capacity, d_tract_id, d_join_type, (UnionTract *) d_tracts);
  st.end ();
  u32 ng = 0;
  rc = read_back (c, fn, scan_total (c, n), &ng, 1);
  if (rc) return -rc;
  if ((long) ng > capacity) return -set_err (TJAMD_ERR_CAPACITY, "%s: %u tracts, caller capacity %ld", fn, ng, capacity);
  st.done ();
  c->union_cand = n_cand;
  return (long) ng;
}

// A sample's bars in a tract: its non-zero rows summed per signed 10-bit length, then the lengths with a non-zero sum in
// the order of the reference's h (count descending, the larger length first on a tie).  Slot q of a lane lives at
// cnt[q * stride], len[q * stride].  FULL: every possible length has a slot (1024, global memory); otherwise the lengths
// are looked up among UT_SLOTS slots (LDS) and -1 says that the sample has more.  Returns the number of bars; integral and
// n_ctx (changes of context between non-zero rows: a tract's rows of one context are contiguous) are the sample's.
#define UT_SLOTS 16
#define UT_LENGTHS 1024
#define UT_FULL_BLOCKS 4

template <bool FULL>
__device__ int union_sample_bars (const u64 *__restrict__ keys, const int *__restrict__ counts, int ns, long first, long end, int s,
                                  long long *cnt, int *len, long stride, long long &integral, int &n_ctx)
{
  int nb = 0;
  long prev = -1;
  integral = 0; n_ctx = 0;
  if (FULL) for (int q = 0; q < UT_LENGTHS; q++) cnt[q * stride] = 0;
  for (long r = first; r < end; r++) {
    const int x = counts[r * ns + s];
    if (x == 0) continue;
    const int l = meta_len (keys[3 * r + 2]);
    if (prev < 0 || !same_context_rows (keys, r, prev)) n_ctx++;
    prev = r;
    integral += x;
    if (FULL) cnt[(l + UT_LENGTHS / 2) * stride] += x;
    else {
      int q = 0;
      while (q < nb && len[q * stride] != l) q++;
      if (q == nb) {
        if (nb == UT_SLOTS) return -1;
        len[q * stride] = l; cnt[q * stride] = 0; nb++;
      }
      cnt[q * stride] += x;
    }
  }
  const int n_slots = FULL ? UT_LENGTHS : nb;
  int b = 0;
  for (int q = 0; q < n_slots; q++) {                   // keep the non-zero sums (b <= q: in place)
    const long long x = cnt[q * stride];
    if (x == 0) continue;
    const int l = FULL ? q - UT_LENGTHS / 2 : len[q * stride];
    cnt[b * stride] = x; len[b * stride] = l; b++;
  }
  for (int a = 1; a < b; a++) {                         // count descending, then length descending (insertion sort)
    const long long x = cnt[a * stride];
    const int l = len[a * stride];
    int q = a - 1;
    while (q >= 0 && (cnt[q * stride] < x || (cnt[q * stride] == x && len[q * stride] < l))) {
      cnt[(q + 1) * stride] = cnt[q * stride]; len[(q + 1) * stride] = len[q * stride]; q--;
    }
    cnt[(q + 1) * stride] = x; len[(q + 1) * stride] = l;
  }
  return b;
}

// descriptive_stats_of_histogram (src/genome_set.c:738-766) on the ordered bars, its sums bar by bar; false if no bar
__device__ bool union_sample_values (const long long *cnt, const int *len, long stride, int nb, long long integral, int n_ctx, int cov,
                                     double *v, int &modal_len)
{
  for (int j = 0; j < TJAMD_N_TRACT_STATS; j++) v[j] = 0.0;
  modal_len = 0;
  if (nb <= 0) return false;
  const double I = (double) integral;
  double avg = 0.0, ent = 0.0;
  for (int q = 0; q < nb; q++) {
    const long long x = cnt[q * stride];
    avg += (double) (x * (long long) len[q * stride]) / I;
    const double p = (double) x / I;
    ent += p * log (p);
  }
  v[TJAMD_STAT_AVG_LENGTH] = avg;
  v[TJAMD_STAT_MODAL_FREQ] = (double) cnt[0] / I;
  v[TJAMD_STAT_PROP_COVERAGE] = I / (double) cov;
  v[TJAMD_STAT_COVERAGE_PER_CONTEXT] = I / (double) n_ctx;
  v[TJAMD_STAT_ENTROPY] = -ent;
  modal_len = len[0];
  return true;
}

// a lane's slots: LDS [UT_SLOTS][256] (the block's threads side by side), or global [UT_LENGTHS][threads of the grid]
#define UT_LANE_SLOTS(FULL, g_cnt, g_len)                                                                            \
  __shared__ long long s_cnt[FULL ? 1 : UT_SLOTS * 256];                                                             \
  __shared__ int s_len[FULL ? 1 : UT_SLOTS * 256];                                                                   \
  const long gthread = blockIdx.x * (long) blockDim.x + threadIdx.x;                                                 \
  long long *cnt = FULL ? g_cnt + gthread : s_cnt + threadIdx.x;                                                     \
  int *len = FULL ? g_len + gthread : s_len + threadIdx.x;                                                           \
  const long stride = FULL ? (long) gridDim.x * blockDim.x : 256l;

// One segment of S lanes per tract, as tract_stats_kernel.  !FULL: every tract; a tract where a sample has more than UT_SLOTS
// lengths is only flagged (fallback[t] = 1).  FULL (UT_FULL_BLOCKS blocks): the flagged tracts.  err[0] |= 1 where the
// tracts do not tile the union (then nothing is read outside it).  Every flag below n_tracts is written.
template <bool FULL>
__global__ __launch_bounds__ (256)
void union_tract_stats_kernel (const u64 *__restrict__ keys, const int *__restrict__ counts, long n_union, int ns, int S, const int *__restrict__ cov,
                               const int *__restrict__ ref_len, const UnionTract *__restrict__ tracts, long n_tracts, UnionSummary *__restrict__ sum,
                               u32 *__restrict__ varflag, u32 *__restrict__ selflag, u32 *__restrict__ fallback,
                               long long *__restrict__ g_cnt, int *__restrict__ g_len, int *__restrict__ err)
{
  UT_LANE_SLOTS (FULL, g_cnt, g_len)
  SEGMENT_MAP (S, lane, first_item, segs_per_grid)
  for (long t = first_item; t < n_tracts; t += segs_per_grid) {   // (uniform across a segment)
    if (FULL && !fallback[t]) continue;
    const UnionTract u = tracts[t];
    const long first = u.first, end = first + (long) u.n_rows;
    if (breaks_tiling (tracts, n_tracts, n_union, t)) {
      if (lane == 0) { atomicOr (err, 1); varflag[t] = 0u; selflag[t] = 0u; if (!FULL) fallback[t] = 0u; }
      continue;
    }
    const int ref = ref_len ? ref_len[t] : 0;
    TractSpread sp;
    int over = 0;
    for (int s = lane; s < ns; s += S) {
      double v[TJAMD_N_TRACT_STATS];
      long long integral;
      int n_ctx, ml;
      const int nb = union_sample_bars<FULL> (keys, counts, ns, first, end, s, cnt, len, stride, integral, n_ctx);
      if (nb < 0) { over = 1; break; }
      if (union_sample_values (cnt, len, stride, nb, integral, n_ctx, cov[s], v, ml)) sp.add (v, ml, ref);
    }
    sp.reduce (S);
    for (int o = 1; o < S; o <<= 1) over |= __shfl_xor (over, o, S);
    if (lane != 0) continue;
    if (!FULL) fallback[t] = (u32) over;
    if (over) { varflag[t] = 0u; selflag[t] = 0u; continue; }   // (FULL never overflows: the fallback kernel writes this tract)
    UnionSummary o;
    o.first = (int) first; o.n_rows = u.n_rows; o.n_present = sp.present; o.lev_distance = u.lev_distance;
    o.variable = sp.finish (ns, o.reldiff);
    o.selected = (sp.present < ns || u.lev_distance > 0 || o.reldiff[TJAMD_STAT_MODAL_FREQ] > 1e-6 ||  // print_selected_g_tract_vector
                  o.reldiff[TJAMD_STAT_AVG_LENGTH] > 1e-6 || o.reldiff[TJAMD_STAT_ENTROPY] > 1e-6) ? 1 : 0;
    sum[t] = o;
    varflag[t] = (u32) o.variable; selflag[t] = (u32) o.selected;
  }
}

// the per-sample values of listed tracts; !FULL flags (fallback[i] = 1) an entry where a sample has more than UT_SLOTS
// lengths, FULL (UT_FULL_BLOCKS blocks) writes the flagged entries again
template <bool FULL>
__global__ __launch_bounds__ (256)
void union_tract_sample_stats_kernel (const u64 *__restrict__ keys, const int *__restrict__ counts, long n_union, int ns, int S, const int *__restrict__ cov,
                                      const UnionSummary *__restrict__ sum, long n_tracts, const int *__restrict__ list, long n_list,
                                      double *__restrict__ values, int *__restrict__ modal_len, int *__restrict__ n_context, int *__restrict__ n_len,
                                      u32 *__restrict__ fallback, long long *__restrict__ g_cnt, int *__restrict__ g_len, int *__restrict__ err)
{
  UT_LANE_SLOTS (FULL, g_cnt, g_len)
  SEGMENT_MAP (S, lane, first_item, segs_per_grid)
  for (long i = first_item; i < n_list; i += segs_per_grid) {
    if (FULL && !fallback[i]) continue;
    long first, end;
    listed_tract_rows (sum, n_tracts, n_union, list[i], lane, err, first, end);
    int over = 0;
    for (int s = lane; s < ns; s += S) {
      double v[TJAMD_N_TRACT_STATS];
      long long integral;
      int n_ctx, ml;
      const int nb = union_sample_bars<FULL> (keys, counts, ns, first, end, s, cnt, len, stride, integral, n_ctx);
      if (nb < 0) { over = 1; break; }
      if (!union_sample_values (cnt, len, stride, nb, integral, n_ctx, cov[s], v, ml)) n_ctx = 0;
      write_listed_sample (i, s, ns, v, ml, n_ctx, values, modal_len, n_context);
      if (n_len) n_len[i * ns + s] = nb;
    }
    if (!FULL) {
      for (int o = 1; o < S; o <<= 1) over |= __shfl_xor (over, o, S);
      if (lane == 0) fallback[i] = (u32) over;
    }
  }
}

static int ensure_union_fallback (tjamd_counter *c, long n, long long *&g_cnt, int *&g_len)
{ // fallback flags, and the global bars of the FULL kernels: g_cnt, the counts of all their threads, then g_len, the lengths
  int rc = ensure (c->ut_fb, (size_t) std::max (n, 1l) * 4, c->stream);
  const size_t threads = (size_t) UT_FULL_BLOCKS * 256;
  if (!rc) rc = ensure (c->ut_slots, threads * UT_LENGTHS * (sizeof (long long) + sizeof (int)), c->stream);
  g_cnt = (long long *) c->ut_slots.p;                  // (null after a failed first allocation: the caller returns)
  g_len = (int *) (g_cnt + threads * UT_LENGTHS);
  return rc;
}

extern "C" long tjamd_union_tract_stats (tjamd_counter *c, const void *d_keys, const void *d_counts, long n_union, int n_samples,
                                         const tjamd_union_tract *d_tracts, long n_tracts, const int *coverage, const int *d_ref_length,
                                         tjamd_union_tract_summary *d_summary, int *d_var, long *n_var, int *d_sel, long *n_sel)
{
  static const char *fn = "tjamd_union_tract_stats";
  int rc = tract_args (fn, d_keys, d_counts, n_union, n_samples, coverage);   // (the coverage before the tracts: not tiled_union_args)
  if (!rc) rc = tract_count_arg (fn, n_tracts, n_union);
  if (rc) return -rc;
  if (n_tracts > 0 && (!d_tracts || !d_summary)) return -set_err (TJAMD_ERR_ARG, "%s: null tract or summary buffer", fn);
  if (!c) return -set_err (TJAMD_ERR_ARG, "%s: null counter", fn);
  if (n_var) *n_var = 0;
  if (n_sel) *n_sel = 0;
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  Stage st (c, T_UNION_STATS);
  if (n_union == 0) return 0;
  const long nt = n_tracts;
  rc = ensure (c->flags, (size_t) nt * 4, c->stream);               // variable flags, then their positions in outpos
  if (!rc) rc = ensure (c->outpos, (size_t) nt * 4, c->stream);
  if (!rc) rc = ensure (c->keep, (size_t) nt * 4, c->stream);      // selected flags, then their positions in headpos
  if (!rc) rc = ensure (c->headpos, (size_t) nt * 4, c->stream);
  if (!rc) rc = ensure (c->scan_tmp, scan_tmp_words (nt) * 4 + 64, c->stream);
  long long *g_cnt = nullptr;
  int *g_len = nullptr;
  if (!rc) rc = ensure_union_fallback (c, nt, g_cnt, g_len);
  if (!rc) rc = upload_coverage (c, coverage, n_samples);
  if (rc) return -rc;
  st.begin ();
  u32 *total = scan_total (c, nt);
  int *err = (int *) c->ts_aux.p;
  const int S = tract_segment (n_samples);
  u32 *vf = (u32 *) c->flags.p, *sf = (u32 *) c->keep.p, *fb = (u32 *) c->ut_fb.p;
  auto launch = [&] (auto kernel, unsigned grid) {
    hipLaunchKernelGGL (kernel, dim3 (grid), dim3 (256), 0, c->stream, (const u64 *) d_keys, (const int *) d_counts, n_union, n_samples, S, (const int *) c->ts_cov.p,
                        d_ref_length, (const UnionTract *) d_tracts, nt, (UnionSummary *) d_summary, vf, sf, fb, g_cnt, g_len, err);
  };
  launch (union_tract_stats_kernel<false>, tract_grid (nt, S));
  launch (union_tract_stats_kernel<true>, (unsigned) UT_FULL_BLOCKS);
  if (hipGetLastError () != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: launch failed", fn);
  rc = exclusive_scan (c, vf, (u32 *) c->outpos.p, nt, total);
  if (!rc) rc = exclusive_scan (c, sf, (u32 *) c->headpos.p, nt, total + 1);
  if (rc) return -rc;
  if (d_var) hipLaunchKernelGGL (tract_var_scatter_kernel, dim3 (grid_for (nt)), dim3 (256), 0, c->stream, (const u32 *) vf, (const u32 *) c->outpos.p, nt, d_var);
  if (d_sel) hipLaunchKernelGGL (tract_var_scatter_kernel, dim3 (grid_for (nt)), dim3 (256), 0, c->stream, (const u32 *) sf, (const u32 *) c->headpos.p, nt, d_sel);
  if (hipGetLastError () != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: list launch failed", fn);
  st.end ();
  int h_err = 0;
  u32 h_tot[2] = {0, 0};
  if (hipMemcpyAsync (&h_err, err, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipMemcpyAsync (h_tot, total, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize (c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: failed: %s", fn, hipGetErrorString (hipGetLastError ()));
  if (h_err) return -set_err (TJAMD_ERR_ARG, "%s: the tracts must tile the union (first 0, each starting where the one before ends, the last ending at row %ld)", fn, n_union);
  st.done ();
  if (n_var) *n_var = (long) h_tot[0];
  if (n_sel) *n_sel = (long) h_tot[1];
  return nt;
}

extern "C" long tjamd_union_tract_sample_stats (tjamd_counter *c, const void *d_keys, const void *d_counts, long n_union, int n_samples,
                                                const int *coverage, const tjamd_union_tract_summary *d_summary, long n_tracts,
                                                const int *d_list, long n_list, double *d_values, int *d_modal_len, int *d_n_context, int *d_n_len)
{
  static const char *fn = "tjamd_union_tract_sample_stats";
  int rc = tract_args (fn, d_keys, d_counts, n_union, n_samples, coverage);
  if (rc) return -rc;
  if (n_list < 0 || n_tracts < 0 || n_tracts > n_union) return -set_err (TJAMD_ERR_ARG, "%s: n_list %ld, n_tracts %ld (union of %ld rows)", fn, n_list, n_tracts, n_union);
  if (n_list > 0 && (!d_summary || !d_list || !d_values)) return -set_err (TJAMD_ERR_ARG, "%s: null summary, list or values buffer", fn);
  if (!c) return -set_err (TJAMD_ERR_ARG, "%s: null counter", fn);
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  if (n_list == 0) return 0;
  long long *g_cnt = nullptr;
  int *g_len = nullptr;
  rc = ensure_union_fallback (c, n_list, g_cnt, g_len);
  if (!rc) rc = upload_coverage (c, coverage, n_samples);
  if (rc) return -rc;
  const int S = tract_segment (n_samples);
  int *err = (int *) c->ts_aux.p, h_err = 0;
  auto launch = [&] (auto kernel, unsigned grid) {
    hipLaunchKernelGGL (kernel, dim3 (grid), dim3 (256), 0, c->stream, (const u64 *) d_keys, (const int *) d_counts, n_union, n_samples, S, (const int *) c->ts_cov.p,
                        (const UnionSummary *) d_summary, n_tracts, d_list, n_list, d_values, d_modal_len, d_n_context, d_n_len, (u32 *) c->ut_fb.p, g_cnt, g_len, err);
  };
  launch (union_tract_sample_stats_kernel<false>, tract_grid (n_list, S));
  launch (union_tract_sample_stats_kernel<true>, (unsigned) UT_FULL_BLOCKS);
  rc = read_back (c, fn, err, &h_err, 1);
  if (rc) return -rc;
  if (h_err) return -set_err (TJAMD_ERR_ARG, "%s: a listed tract id is outside [0, %ld) or its rows outside the union", fn, n_tracts);
  return n_list;
}

// first launch to last of the last tjamd_union_tracts, the host's wait for the retry candidates included
TJ_LAST_MS (tjamd_last_union_tracts_ms, T_UNION)

extern "C" long tjamd_last_union_tract_candidates (tjamd_counter *c) { return c ? c->union_cand : -1; }

TJ_LAST_MS (tjamd_last_union_tract_stats_ms, T_UNION_STATS)

// Peer access between two devices of this process, asked for once per ordered pair: with it hipMemcpyPeerAsync moves the
// bytes over xGMI directly, without it the runtime stages them through host memory.  Returns 1 direct, 0 staged;
// tjamd_peer_access_report () says which pairs are which.
static std::mutex g_peer_mutex;
static signed char g_peer[64][64];                      // 0 unknown, 1 direct, -1 refused
static int peer_access (int dst_dev, int src_dev)
{
  if (dst_dev == src_dev) return 1;
  if (dst_dev < 0 || src_dev < 0 || dst_dev >= 64 || src_dev >= 64) return 0;
  std::lock_guard<std::mutex> lock (g_peer_mutex);
  if (g_peer[dst_dev][src_dev]) return g_peer[dst_dev][src_dev] > 0;
  int can = 0, prev = -1;
  (void) hipGetDevice (&prev);
  if (hipDeviceCanAccessPeer (&can, dst_dev, src_dev) == hipSuccess && can && hipSetDevice (dst_dev) == hipSuccess) {
    const hipError_t e = hipDeviceEnablePeerAccess (src_dev, 0);
    can = (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled);
    (void) hipGetLastError ();
  }
  else can = 0;
  if (prev >= 0) (void) hipSetDevice (prev);
  g_peer[dst_dev][src_dev] = can ? 1 : -1;
  return can;
}

extern "C" int tjamd_peer_access_report (char *out, int capacity)
{ // "dst<-src:direct" / "dst<-src:staged" for every pair a gather has used so far; returns the number of staged pairs
  int staged = 0, at = 0;
  std::lock_guard<std::mutex> lock (g_peer_mutex);
  if (out && capacity > 0) out[0] = 0;
  for (int d = 0; d < 64; d++)
    for (int sdev = 0; sdev < 64; sdev++)
      if (g_peer[d][sdev]) {
        if (g_peer[d][sdev] < 0) staged++;
        if (out && at < capacity - 24) at += snprintf (out + at, (size_t) (capacity - at), "%d<-%d:%s ", d, sdev, g_peer[d][sdev] > 0 ? "direct" : "staged");
      }
  return staged;
}

// The exchange of the cross-sample merge for a caller that, like the reference, runs its samples as threads of ONE
// process (src/genome_set.c:66-94; merge at :195-229): the kept records of the finalised counters `samples` -- each on
// the device its thread bound it to -- are copied into one buffer on dst's device (peer copies over xGMI between
// devices, a plain device copy on the same one), back to back in sample order.  counts[i] = records of sample i;
// *d_records = the buffer (owned by dst, valid until its next gather).  Returns the total, ready for
// tjamd_merge_samples (dst, *d_records, counts, n_samples, ...).
extern "C" long tjamd_gather_histograms (tjamd_counter *dst, tjamd_counter *const *samples, int n_samples, const void **d_records, long *counts)
{
  if (!dst || !samples || n_samples < 1 || !d_records || !counts) return -set_err (TJAMD_ERR_ARG, "bad arguments");
  long n = 0;
  for (int i = 0; i < n_samples; i++) {
    if (!samples[i] || samples[i]->status < 0) return -set_err (TJAMD_ERR_STATE, "sample %d is not finalised", i);
    counts[i] = samples[i]->n_kept; n += counts[i];
  }
  if (hipSetDevice (dst->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  int rc = ensure (dst->rawlist, (size_t) std::max<long> (n, 1) * 24, dst->stream);
  if (rc) return -rc;
  size_t off = 0;
  for (int i = 0; i < n_samples; i++) {
    const size_t bytes = (size_t) counts[i] * 24;
    if (!bytes) continue;
    tjamd_counter *s = samples[i];
    if (s->device != dst->device) peer_access (dst->device, s->device);   // (direct xGMI copies; staged through the host by the runtime where it is refused)
    hipError_t e = (s->device == dst->device)
      ? hipMemcpyAsync ((char *) dst->rawlist.p + off, s->kept.p, bytes, hipMemcpyDeviceToDevice, dst->stream)
      : hipMemcpyPeerAsync ((char *) dst->rawlist.p + off, dst->device, s->kept.p, s->device, bytes, dst->stream);
    if (e != hipSuccess) return -set_err (TJAMD_ERR_HIP, "gather copy of sample %d failed: %s", i, hipGetErrorString (e));
    off += bytes;
  }
  if (hipStreamSynchronize (dst->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "gather failed");
  *d_records = dst->rawlist.p;
  return n;
}


extern "C" long tjamd_merge_samples (tjamd_counter *c, const void *d_records, const long *counts, int n_samples,
                                      void *d_out_keys, void *d_out_counts, long capacity)
{
  if (!c || !counts || n_samples < 1 || n_samples > 4096 || !d_out_keys || !d_out_counts) return -set_err (TJAMD_ERR_ARG, "bad arguments");
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  std::vector<long> starts ((size_t) n_samples + 1);
  long n = 0;
  for (int i = 0; i < n_samples; i++) { if (counts[i] < 0) return -set_err (TJAMD_ERR_ARG, "negative count"); starts[i] = n; n += counts[i]; }
  starts[n_samples] = n;
  if (n == 0) return 0;
  if (!d_records) return -set_err (TJAMD_ERR_ARG, "null records");
  if (n >= (1l << 31)) return -set_err (TJAMD_ERR_CAPACITY, "%ld records to merge", n);

  // bins of ~32..64 records: partition, then one wavefront per bin finds the distinct keys, their order and depths
  int nbits = 6;
  while (nbits < BS_MAXBITS && nbits < 1 + 4 * c->k && (24l << nbits) < n) nbits++;   // (the per-bin work is quadratic in the bin's size: bins of ~30 records)
  nbits = std::min (nbits, 1 + 4 * c->k);
  const int nbins = 1 << nbits;
  int rc = ensure (c->prefix, (size_t) (n_samples + 1) * 8, c->stream);
  if (!rc) rc = ensure (c->alt, (size_t) n * 24, c->stream);
  if (!rc && !c->bins.p) { rc = ensure (c->bins, (size_t) (BS_MAXBINS + 1) * 4, c->stream); c->bins_zeroed = false; }
  if (!rc) rc = ensure (c->binstart, (size_t) (BS_MAXBINS + 1) * 4, c->stream);
  if (!rc) rc = ensure (c->binctx, (size_t) BS_MAXBINS * 8, c->stream);
  if (!rc) rc = ensure (c->headpos, (size_t) n * 4, c->stream);
  if (!rc) rc = ensure (c->outpos, (size_t) n * 4, c->stream);
  if (rc) return -rc;
  if (hipMemcpyAsync (c->prefix.p, starts.data (), (size_t) (n_samples + 1) * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize (c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "copy failed");
  u32 *bins = (u32 *) c->bins.p, *binstart = (u32 *) c->binstart.p, *binctx = (u32 *) c->binctx.p, *binout = binctx + nbins;
  u32 *tpos = (u32 *) c->headpos.p, *ttot = (u32 *) c->outpos.p;
  if (!c->bins_zeroed && hipMemsetAsync (bins, 0, (size_t) BS_MAXBINS * 4, c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "memset failed");
  c->bins_zeroed = false;
  Stage st (c, T_MERGE);
  st.begin ();
  hipLaunchKernelGGL (bin_count_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const u64 *) d_records, n, c->k, nbits, bins, (uint4 *) nullptr, 0l, 1);
  hipLaunchKernelGGL (bin_scan_kernel, dim3 (1), dim3 (WGS_THREADS), 0, c->stream, bins, nbins, binstart,
                      c->bin_rank_max < (u32) BS_RANK_MAX ? c->bin_rank_max : (u32) MG_RANK_MAX, c->d_fin);   // (test hook: see TATAJUBA_AMD_BIN_MAX)
  hipLaunchKernelGGL (merge_scatter_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const u64 *) d_records, (u64 *) c->alt.p, n, c->k, nbits, bins,
                      (const long *) c->prefix.p, n_samples);
  hipLaunchKernelGGL (bin_merge_kernel, dim3 ((unsigned) std::min (nbins, 16384)), dim3 (64), 0, c->stream, (const u64 *) c->alt.p, (const u32 *) binstart, nbins,
                      (const FinCounts *) c->d_fin, binctx, tpos, ttot);
  hipLaunchKernelGGL (bin_ctx_scan_kernel, dim3 (1), dim3 (WGS_THREADS), 0, c->stream, (const u32 *) binctx, nbins, binout, c->d_fin);
  hipLaunchKernelGGL (bin_merge_write_kernel, dim3 ((unsigned) std::min (nbins / 4 + 1, 4096)), dim3 (256), 0, c->stream, (const u64 *) c->alt.p, (const u32 *) binstart,
                      (const u32 *) binout, nbins, (const FinCounts *) c->d_fin, (const u32 *) tpos, (const u32 *) ttot, n_samples,
                      (u64 *) d_out_keys, (int *) d_out_counts, capacity);
  if (hipGetLastError () != hipSuccess) return -set_err (TJAMD_ERR_HIP, "merge launch failed");
  st.end ();
  st.done ();                                           // (the merge's own time, whatever the read-back below finds)
  if (hipMemcpyAsync (c->h_fin, c->d_fin, sizeof (FinCounts), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize (c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "merge failed: %s", hipGetErrorString (hipGetLastError ()));
  if (c->h_fin->sort_fallback) return merge_samples_radix (c, d_records, n, n_samples, d_out_keys, d_out_counts, capacity);
  const long n_union = c->h_fin->n_idx;
  if (n_union > capacity) return -set_err (TJAMD_ERR_CAPACITY, "%ld union keys, caller capacity %ld", n_union, capacity);
  return n_union;
}

static long merge_samples_radix (tjamd_counter *c, const void *d_records, long n, int n_samples, void *d_out_keys, void *d_out_counts, long capacity)
{
  int rc = ensure (c->rawlist, (size_t) n * 24, c->stream);
  if (!rc) rc = ensure (c->alt, (size_t) n * 24, c->stream);
  if (!rc) rc = ensure (c->flags, (size_t) n * 4, c->stream);
  if (!rc) rc = ensure (c->segid, (size_t) n * 4, c->stream);
  if (!rc) rc = ensure (c->keep, (size_t) n * 8, c->stream);          // totals per union key, then their flags
  if (!rc) rc = ensure (c->scan_tmp, scan_tmp_words (n) * 4, c->stream);
  if (rc) return -rc;
  hipLaunchKernelGGL (merge_tag_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const u64 *) d_records, (u64 *) c->rawlist.p, n, (const long *) c->prefix.p, n_samples);
  u64 *a = (u64 *) c->rawlist.p, *b = (u64 *) c->alt.p;
  rc = radix_sort_records (c, a, b, n);               // the reference's order; the sample tag does not take part
  if (rc) return -rc;
  if (a != (u64 *) c->rawlist.p) std::swap (c->rawlist, c->alt);
  u32 *flags = (u32 *) c->flags.p, *segid = (u32 *) c->segid.p;
  hipLaunchKernelGGL (seg_heads_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const u64 *) a, n, flags, 0);
  rc = exclusive_scan (c, flags, segid, n, &c->d_fin->n_seg);
  if (rc) return -rc;
  if (hipMemcpyAsync (c->h_fin, c->d_fin, sizeof (FinCounts), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize (c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "merge failed: %s", hipGetErrorString (hipGetLastError ()));
  const long n_union = c->h_fin->n_seg;
  if (n_union > capacity) return -set_err (TJAMD_ERR_CAPACITY, "%ld union keys, caller capacity %ld", n_union, capacity);
  if (hipMemsetAsync (d_out_counts, 0, (size_t) n_union * n_samples * 4, c->stream) != hipSuccess ||
      hipMemsetAsync (c->keep.p, 0, (size_t) n * 8, c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "memset failed");
  hipLaunchKernelGGL (merge_write_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const u64 *) a, n, (const u32 *) flags, (const u32 *) segid,
                      n_samples, (u64 *) d_out_keys, (int *) d_out_counts, (u32 *) c->keep.p, (u32 *) c->keep.p + n, capacity);
  hipLaunchKernelGGL (merge_totals_kernel, dim3 (grid_for (n_union)), dim3 (256), 0, c->stream, (u64 *) d_out_keys, (const u32 *) c->keep.p,
                      (const u32 *) c->keep.p + n, (const u32 *) &c->d_fin->n_seg, capacity);
  if (hipGetLastError () != hipSuccess || hipStreamSynchronize (c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "merge kernels failed");
  return n_union;
}


// ---------------------------------------------------------------------------------------------------------------
// The exchange between PROCESSES, one per GPU: an all-gatherv of the finalised counters' kept records over RCCL (xGMI on
// the node), so that every rank holds every sample's histogram for the cross-sample merge (reference attach point:
// src/genome_set.c:195-229 -- there the samples are threads of one process and the "exchange" is a pointer).
// RCCL has no all-gatherv: every rank contributes one block of the same size -- a header with its record count, then its
// records -- to ONE ncclAllGather on the counter's stream, and a kernel packs the received blocks back to back.  The block
// size is agreed without talking: it is a function of the counts of the exchange before (the same numbers on every
// rank); the first exchange, and one in which some rank holds more than a block takes, learn the counts with an 8-byte
// all-gather first.  One host synchronisation per exchange (the counts the caller gets back), on the usual path.

struct tjamd_comm
{
  ncclComm_t comm = nullptr;
  int rank = 0, world = 1, device = 0;
  long cap = 0;                                         // records per block, 0 = not agreed yet
  hipStream_t stream = nullptr;                         // tjamd_comm_set_stream; null: the stream of the counter being exchanged
  DevBuf send, recv, out, dcounts;
  long *h_counts = nullptr;                             // pinned, world entries
  long exchanges = 0, collectives = 0;
  // the last exchange, for whoever reports on it (bench.py): device time from the first pack to the last unpack (HIP events on
  // the exchange's stream), bytes received, collectives it took (1 when the block size was settled, 2 or more otherwise)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double last_ms = -1.0; long last_bytes = 0, last_collectives = 0;
};

// RCCL is looked up when the first communicator call needs it (dlopen), not when the library is loaded: the one-GPU drop-in
// has no use for it and must load on a machine without it.  <rccl/rccl.h> gives the types; the seven entry points used:
struct RcclApi
{
  const char *(*GetErrorString) (ncclResult_t);
  ncclResult_t (*GetUniqueId) (ncclUniqueId *);
  ncclResult_t (*CommInitRank) (ncclComm_t *, int, ncclUniqueId, int);
  ncclResult_t (*CommDestroy) (ncclComm_t);
  ncclResult_t (*CommCount) (const ncclComm_t, int *);
  ncclResult_t (*CommAbort) (ncclComm_t);
  ncclResult_t (*AllGather) (const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t);
};

static const RcclApi *rccl_api ()
{ // TATAJUBA_AMD_RCCL names the library; otherwise the loader's search path, then $ROCM_PATH/lib (default /opt/rocm/lib)
  static RcclApi api;
  static bool ok = false;
  static char why[512] = "";
  static std::once_flag once;
  std::call_once (once, [] () {
    void *h = nullptr;
    std::string tried;
    std::vector<std::string> names;
    if (const char *e = getenv ("TATAJUBA_AMD_RCCL")) names.push_back (e);
    else {
      names.push_back ("librccl.so.1"); names.push_back ("librccl.so");
      const char *rp = getenv ("ROCM_PATH");
      const std::string root = (rp && *rp) ? rp : "/opt/rocm";
      names.push_back (root + "/lib/librccl.so.1"); names.push_back (root + "/lib/librccl.so");
    }
    for (const std::string &nm : names) {
      h = dlopen (nm.c_str (), RTLD_NOW | RTLD_LOCAL);
      if (h) break;
      tried += (tried.empty () ? "" : ", ") + nm;
    }
    if (!h) { snprintf (why, sizeof why, "RCCL not found (tried %s): the exchange between processes needs it", tried.c_str ()); return; }
    struct { const char *name; void **to; } syms[] = {
      {"ncclGetErrorString", (void **) &api.GetErrorString}, {"ncclGetUniqueId", (void **) &api.GetUniqueId},
      {"ncclCommInitRank", (void **) &api.CommInitRank}, {"ncclCommDestroy", (void **) &api.CommDestroy},
      {"ncclCommCount", (void **) &api.CommCount}, {"ncclCommAbort", (void **) &api.CommAbort}, {"ncclAllGather", (void **) &api.AllGather}};
    for (auto &sy : syms) {
      *sy.to = dlsym (h, sy.name);
      if (!*sy.to) { snprintf (why, sizeof why, "RCCL: %s not found in the library that was loaded", sy.name); return; }
    }
    ok = true;
  });
  if (!ok) { set_err (TJAMD_ERR_HIP, "%s", why); return nullptr; }
  return &api;
}

#define NCCLCHK(name, call, ret) do { ncclResult_t r_ = (call); if (r_ != ncclSuccess) { \
  set_err (TJAMD_ERR_HIP, "%s failed: %s", name, NC->GetErrorString (r_)); return ret; } } while (0)

extern "C" int tjamd_comm_unique_id (void *id_bytes)
{
  static_assert (TJAMD_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
  if (!id_bytes) return set_err (TJAMD_ERR_ARG, "tjamd_comm_unique_id: null buffer");
  const RcclApi *NC = rccl_api ();
  if (!NC) return TJAMD_ERR_HIP;
  ncclUniqueId id;
  NCCLCHK ("ncclGetUniqueId", NC->GetUniqueId (&id), TJAMD_ERR_HIP);
  memcpy (id_bytes, &id, sizeof id);
  return TJAMD_OK;
}

extern "C" tjamd_comm *tjamd_comm_create (tjamd_counter *c, const void *id_bytes, int rank, int world)
{
  if (!c || !id_bytes || world < 1 || world > 4096 || rank < 0 || rank >= world) { set_err (TJAMD_ERR_ARG, "tjamd_comm_create: bad arguments"); return NULL; }
  const RcclApi *NC = rccl_api ();
  if (!NC) return NULL;
  HIPCHK_NULL (hipSetDevice (c->device));
  tjamd_comm *m = new (std::nothrow) tjamd_comm;
  if (!m) { set_err (TJAMD_ERR_HIP, "out of memory"); return NULL; }
  m->rank = rank; m->world = world; m->device = c->device;
  ncclUniqueId id;
  memcpy (&id, id_bytes, sizeof id);
  ncclResult_t r = NC->CommInitRank (&m->comm, world, id, rank);
  if (r != ncclSuccess) { set_err (TJAMD_ERR_HIP, "ncclCommInitRank failed: %s", NC->GetErrorString (r)); delete m; return NULL; }
  if (hipHostMalloc ((void **) &m->h_counts, (size_t) world * sizeof (long), hipHostMallocDefault) != hipSuccess ||
      hipEventCreate (&m->ev0) != hipSuccess || hipEventCreate (&m->ev1) != hipSuccess) {
    set_err (TJAMD_ERR_HIP, "hipHostMalloc / hipEventCreate failed"); (void) NC->CommDestroy (m->comm); delete m; return NULL;
  }
  return m;
}

extern "C" void tjamd_comm_destroy (tjamd_comm *m)
{
  if (!m) return;
  (void) hipSetDevice (m->device);
  if (m->comm) if (const RcclApi *NC = rccl_api ()) (void) NC->CommDestroy (m->comm);
  release (m->send); release (m->recv); release (m->out); release (m->dcounts);
  if (m->h_counts) (void) hipHostFree (m->h_counts);
  if (m->ev0) (void) hipEventDestroy (m->ev0);
  if (m->ev1) (void) hipEventDestroy (m->ev1);
  delete m;
}

extern "C" int tjamd_comm_set_stream (tjamd_comm *m, void *hip_stream)
{
  if (!m) return set_err (TJAMD_ERR_ARG, "tjamd_comm_set_stream: null communicator");
  m->stream = (hipStream_t) hip_stream;
  return TJAMD_OK;
}
extern "C" int tjamd_comm_rank (const tjamd_comm *m) { return m ? m->rank : -1; }
extern "C" int tjamd_comm_world (const tjamd_comm *m) { return m ? m->world : -1; }
// the number of ranks RCCL itself says the communicator has (ncclCommCount), not the argument tjamd_comm_create was given
extern "C" int tjamd_comm_count (const tjamd_comm *m)
{
  int n = -1;
  const RcclApi *NC = (m && m->comm) ? rccl_api () : nullptr;
  if (!NC || NC->CommCount (m->comm, &n) != ncclSuccess) return -1;
  return n;
}
// the last exchange on this communicator: device milliseconds (pack, collective(s), unpack), bytes the data collective
// delivered to this rank, collectives it took.  Any pointer may be NULL.  Returns 0, or non-zero before the first exchange.
extern "C" int tjamd_comm_last_exchange (const tjamd_comm *m, double *ms, long *bytes, long *collectives)
{
  if (!m || m->exchanges == 0 || m->last_collectives == 0) return 1;
  if (ms) *ms = m->last_ms;
  if (bytes) *bytes = m->last_bytes;
  if (collectives) *collectives = m->last_collectives;
  return 0;
}
extern "C" long tjamd_comm_collectives (const tjamd_comm *m) { return m ? m->collectives : -1; }

#define GX_HEADER 16                                    // bytes in front of a block's records: the record count, then padding

__global__ void gx_pack_kernel (const u64 *__restrict__ kept, long n, long cap, u64 *__restrict__ block)
{ // header + the first min (n, cap) records
  const long words = 3 * min (n, cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) { block[0] = (u64) n; block[1] = 0; }
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < words; i += (long) gridDim.x * blockDim.x) block[2 + i] = kept[i];
}

__global__ void gx_unpack_kernel (const u64 *__restrict__ recv, long block_words, int world, long cap, u64 *__restrict__ out, long *__restrict__ counts)
{ // blocks -> records back to back in rank order; counts[r] = what rank r holds (may exceed cap: the caller looks)
  for (int r = blockIdx.y; r < world; r += gridDim.y) {
    long before = 0;
    for (int q = 0; q < r; q++) before += min ((long) recv[(long) q * block_words], cap);
    const u64 *src = recv + (long) r * block_words;
    const long n = (long) src[0], words = 3 * min (n, cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[r] = n;
    for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < words; i += (long) gridDim.x * blockDim.x) out[3 * before + i] = src[2 + i];
  }
}

static long gx_block_cap (long max_count)
{ // what a block takes after an exchange whose fullest rank held max_count: a quarter more, in steps of 4096 records
  const long want = max_count + max_count / 4 + 1;
  return ((want + 4095) / 4096) * 4096;
}

// Test hook (not in the public header): the exchange's pack and unpack kernels on fabricated data -- what the ranks r > 0 of
// a communicator would have sent -- on one GPU.  samples[r] / n[r]: rank r's kept records (host, 3 words each); every rank's
// block is packed with gx_pack_kernel for a block of `cap` records and the blocks are unpacked as tjamd_allgather_histograms
// unpacks what ncclAllGather delivers.  out: world * cap records (host); counts[r] = what rank r says it holds (n[r], also
// when it exceeds cap: the caller's cue to agree on a larger block).  Returns the records unpacked (sum of min (n[r], cap)).
extern "C" long tjamd_debug_exchange_pack_unpack (tjamd_counter *c, const u64 *const *samples, const long *n, int world, long cap, u64 *out, long *counts)
{
  if (!c || !samples || !n || world < 1 || cap < 1 || !out || !counts) return -set_err (TJAMD_ERR_ARG, "bad arguments");
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  const long block_words = GX_HEADER / 8 + 3 * cap;
  u64 *d_kept = nullptr, *d_recv = nullptr, *d_out = nullptr; long *d_counts = nullptr;
  long total = 0, mx = 1;
  for (int r = 0; r < world; r++) mx = std::max (mx, n[r]);
  if (hipMalloc ((void **) &d_kept, (size_t) mx * 24) != hipSuccess || hipMalloc ((void **) &d_recv, (size_t) block_words * 8 * (size_t) world) != hipSuccess ||
      hipMalloc ((void **) &d_out, (size_t) cap * world * 24) != hipSuccess || hipMalloc ((void **) &d_counts, (size_t) world * sizeof (long)) != hipSuccess)
    return -set_err (TJAMD_ERR_HIP, "hipMalloc failed");
  for (int r = 0; r < world; r++) {
    if (n[r] && hipMemcpyAsync (d_kept, samples[r], (size_t) n[r] * 24, hipMemcpyHostToDevice, c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "copy failed");
    hipLaunchKernelGGL (gx_pack_kernel, dim3 (grid_for (3 * std::min (n[r], cap) + 1)), dim3 (256), 0, c->stream, (const u64 *) d_kept, n[r], cap, d_recv + (size_t) r * block_words);
    if (hipStreamSynchronize (c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "pack failed");
    total += std::min (n[r], cap);
  }
  hipLaunchKernelGGL (gx_unpack_kernel, dim3 (grid_for (3 * cap + 1), (unsigned) std::min (world, 64)), dim3 (256), 0, c->stream, (const u64 *) d_recv, block_words, world, cap, d_out, d_counts);
  if (hipMemcpyAsync (out, d_out, (size_t) total * 24, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipMemcpyAsync (counts, d_counts, (size_t) world * sizeof (long), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize (c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "unpack failed: %s", hipGetErrorString (hipGetLastError ()));
  (void) hipFree (d_kept); (void) hipFree (d_recv); (void) hipFree (d_out); (void) hipFree (d_counts);
  return total;
}

extern "C" long tjamd_allgather_histograms (tjamd_counter *c, tjamd_comm *m, const void **d_records, long *counts)
{
  if (!c || !m || !d_records || !counts) return -set_err (TJAMD_ERR_ARG, "tjamd_allgather_histograms: bad arguments");
  if (c->status < 0) return -set_err (TJAMD_ERR_STATE, "tjamd_allgather_histograms needs a finalised counter");
  if (c->device != m->device) return -set_err (TJAMD_ERR_ARG, "the communicator was made for device %d, the counter lives on %d", m->device, c->device);
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  if (!m->comm) return -set_err (TJAMD_ERR_STATE, "the communicator was aborted after a failed exchange");
  const RcclApi *NC = rccl_api ();                      // (there: the communicator was made through it)
  if (!NC) return -TJAMD_ERR_HIP;
  const int world = m->world;
  const long n_mine = c->n_kept;
  // A rank that gives up between two collectives would leave its peers waiting in theirs for ever: every failure from
  // here on aborts the communicator (ncclCommAbort: the peers' pending and later calls fail instead of hanging).
  auto give_up = [&] (int code) -> long { if (m->comm) { (void) NC->CommAbort (m->comm); m->comm = nullptr; } return -(long) code; };
  // (a stream of the communicator's own: the exchange of a finalised sample runs beside the scan of the next one; the
  // caller has seen this counter's finalise end -- tjamd_finalise / tjamd_finalise_end -- so its kept records are complete)
  const hipStream_t st = m->stream ? m->stream : c->stream;
  int rc = ensure (m->dcounts, (size_t) (world + 1) * sizeof (long), st);
  if (rc) return give_up (rc);
  long *d_counts = (long *) m->dcounts.p;
  m->exchanges++;
  const long collectives_before = m->collectives;
  (void) hipEventRecord (m->ev0, st);
  for (int attempt = 0; attempt < 3; attempt++) {
    if (m->cap == 0) {                                  // block size not agreed (first exchange, or the last one overflowed): the counts first
      if (hipMemcpyAsync (d_counts + world, &n_mine, sizeof (long), hipMemcpyHostToDevice, st) != hipSuccess) return give_up (set_err (TJAMD_ERR_HIP, "copy failed"));
      NCCLCHK ("ncclAllGather (counts)", NC->AllGather (d_counts + world, d_counts, sizeof (long), ncclChar, m->comm, st), -TJAMD_ERR_HIP);
      m->collectives++;
      if (hipMemcpyAsync (m->h_counts, d_counts, (size_t) world * sizeof (long), hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize (st) != hipSuccess) return give_up (set_err (TJAMD_ERR_HIP, "exchange of the counts failed: %s", hipGetErrorString (hipGetLastError ())));
      long mx = 0;
      for (int r = 0; r < world; r++) mx = std::max (mx, m->h_counts[r]);
      m->cap = gx_block_cap (mx);
    }
    const long cap = m->cap, block_words = GX_HEADER / 8 + 3 * cap;
    rc = ensure (m->send, (size_t) block_words * 8, st);
    if (!rc) rc = ensure (m->recv, (size_t) block_words * 8 * (size_t) world, st);
    if (!rc) rc = ensure (m->out, (size_t) std::max<long> (cap * world, 1) * 24, st);
    if (rc) return give_up (rc);
    hipLaunchKernelGGL (gx_pack_kernel, dim3 (grid_for (3 * std::min (n_mine, cap) + 1)), dim3 (256), 0, st, (const u64 *) c->kept.p, n_mine, cap, (u64 *) m->send.p);
    NCCLCHK ("ncclAllGather", NC->AllGather (m->send.p, m->recv.p, (size_t) block_words * 8, ncclChar, m->comm, st), -TJAMD_ERR_HIP);
    m->collectives++;
    hipLaunchKernelGGL (gx_unpack_kernel, dim3 (grid_for (3 * cap + 1), (unsigned) std::min (world, 64)), dim3 (256), 0, st,
                        (const u64 *) m->recv.p, block_words, world, cap, (u64 *) m->out.p, d_counts);
    if (hipGetLastError () != hipSuccess) return give_up (set_err (TJAMD_ERR_HIP, "exchange launch failed"));
    (void) hipEventRecord (m->ev1, st);
    if (hipMemcpyAsync (m->h_counts, d_counts, (size_t) world * sizeof (long), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize (st) != hipSuccess) return give_up (set_err (TJAMD_ERR_HIP, "exchange failed: %s", hipGetErrorString (hipGetLastError ())));
    long mx = 0, total = 0;
    for (int r = 0; r < world; r++) { mx = std::max (mx, m->h_counts[r]); total += m->h_counts[r]; }
    if (mx > cap) { m->cap = 0; continue; }             // (every rank sees the same counts and takes the same turn)
    m->cap = gx_block_cap (mx);
    for (int r = 0; r < world; r++) counts[r] = m->h_counts[r];
    *d_records = m->out.p;
    {
      float ms = 0.f;
      m->last_ms = hipEventElapsedTime (&ms, m->ev0, m->ev1) == hipSuccess ? (double) ms : -1.0;
      m->last_bytes = block_words * 8 * (long) world;     // (what the data collective moved into this rank: every rank's max-padded block)
      m->last_collectives = m->collectives - collectives_before;
    }
    return total;
  }
  return -set_err (TJAMD_ERR_STATE, "the exchange did not settle on a block size");
}

// ---------------------------------------------------------------------------------------------------------------
// N7: tracts located on a reference genome by flank matching (reference: find_reference_location_and_sort_hopo_counter,
// src/hopo_counter.c:495-572, which asks BWA; find_best_context_name_for_reference, src/genome_set.c:525-577, which rescans
// the reference window; context_histograms_overlap / genomic_context_merge_histograms_at_same_location,
// src/context_histogram.c:88-110,364-385, which make one tract of two histograms at one place).  The genome is scanned as
// a stream of reads: a tract seen in a read and the same tract seen in the genome give the same canonical (base, ctx0,
// ctx1), so locating is a join of keys against an index of the genome's own runs, one flank exact and the other within
// max_mismatches.  Three parts: the index (tjamd_reference), the lookup (tjamd_locate), the tracts merged by location
// (tjamd_located_tracts).  DESIGN.md section 3.5, N7, has the layout, the thread mapping of the lookup and the measurements.

struct RefEntry { u64 ctx0, ctx1; long long flat; int contig, pos, length, base, neg_strand, pad; };
static_assert (sizeof (RefEntry) == 48 && sizeof (RefEntry) == sizeof (tjamd_ref_entry), "reference entry layout");
struct Location { long long flat; int contig, pos, ref_length, mismatches, neg_strand, n_hits; };
static_assert (sizeof (Location) == 32 && sizeof (Location) == sizeof (tjamd_location), "location layout");
#define LC_NOWHERE Location {-1, -1, -1, 0, 0, 0, 0}     // a row or a tract that has no location: flat, contig and pos -1, the rest 0

// The two orders of the index are arrays of three-word records (primary flank, secondary flank, word) sorted by
// radix_sort_records: descending by (base, primary, secondary), entries of one key in ascending entry number -- which is
// ascending flat position, the entries being written in stream order.  The word holds the base in bits 0-1, where the
// sort key reads it, and the entry number in bits 12-43 (the count and mismatch fields, which the sort key does not read).
#define LC_IDX_SHIFT 12
#define LC_PAD_IDX   0xFFFFFFFFull      // a record beyond the last entry: smallest key, behind every entry (the sort is stable)

struct tjamd_reference
{
  int device = 0, k = 0;
  long n_entries = 0, n_contigs = 0;
  RefEntry *entries = nullptr;          // ascending flat
  u64 *ord[2] = {nullptr, nullptr};     // [0]: primary = ctx0, secondary = ctx1; [1]: the other way round
  void *owned[4] = {nullptr, nullptr, nullptr, nullptr};
  u64 *seed = nullptr;                  // N10 (tjamd_reference_add_seeds): primary = rev_k (ctx1), secondary = ctx0; a block of its own
  bool has_seeds = false;
};

// a handle (`what`: its noun; N7's reference, N9's annotation, N11's coding table) lives on the counter's device
static int on_counter_device (const char *fn, const char *what, int device, const tjamd_counter *c)
{
  return device == c->device ? TJAMD_OK : set_err (TJAMD_ERR_ARG, "%s: the %s lives on device %d, the counter on device %d", fn, what, device, c->device);
}
static int reference_of_counter (const char *fn, const tjamd_reference *ref, const tjamd_counter *c)
{ // the reference belongs to the counter: the same k, the same device (neither is null)
  if (ref->k != c->k) return set_err (TJAMD_ERR_ARG, "%s: the reference was built with k = %d, the counter has k = %d", fn, ref->k, c->k);
  return on_counter_device (fn, "reference", ref->device, c);
}

// A genome stream from the host (N7's index, N11's coding table).  stream_refused: what can be said of it without a device, 0 or
// the code with the message set.  upload_stream: its bytes into c->stage, grown here (which may wait for the counter's stream).
static int stream_refused (const char *fn, const void *h_stream, size_t n_bytes)
{
  if (n_bytes && !h_stream) return set_err (TJAMD_ERR_ARG, "%s: null stream", fn);
  return n_bytes < (size_t) 1 << 31 ? TJAMD_OK : set_err (TJAMD_ERR_CAPACITY, "%s: a stream of %zu bytes (positions are 32-bit)", fn, n_bytes);
}
static int upload_stream (tjamd_counter *c, const char *fn, const void *h_stream, size_t n_bytes)
{
  const int rc = ensure (c->stage, (n_bytes + 255) & ~(size_t) 255, c->stream);
  if (rc || !n_bytes) return rc;
  return hipMemcpyAsync (c->stage.p, h_stream, n_bytes, hipMemcpyHostToDevice, c->stream) == hipSuccess ? TJAMD_OK : set_err (TJAMD_ERR_HIP, "%s: copy to device failed", fn);
}

// Feature i of a host array against the number of contigs it may name (N9's table, N11's): 0, or the code with the message set.
// (Per feature: N9's own rule, cls, keeps its place between one feature and the next.)
static int feature_refused (const char *fn, long i, const tjamd_feature &x, long n_contigs)
{
  if (x.contig < 0 || (long) x.contig >= n_contigs) return set_err (TJAMD_ERR_ARG, "%s: feature %ld: contig %d outside [0, %ld)", fn, i, x.contig, n_contigs);
  if (x.start < 1) return set_err (TJAMD_ERR_ARG, "%s: feature %ld: start %d < 1", fn, i, x.start);
  return x.end >= x.start ? TJAMD_OK : set_err (TJAMD_ERR_ARG, "%s: feature %ld: end %d < start %d", fn, i, x.end, x.start);
}

// byte classes of the index: 0-3 the base of an ACGTU byte (either case), 4 the contig delimiter, 5 anything else
__device__ __forceinline__ u32 ref_class (u32 b) { return byte_is_acgtu (b) ? byte_code (b) : (b == '\n' ? 4u : 5u); }

// a segment is a maximal stretch of one class; every delimiter is a segment of its own (an empty contig still counts)
__global__ void ref_seg_flag_kernel (const uint8_t *__restrict__ seq, long n, u32 *__restrict__ flag)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    const u32 cl = ref_class (seq[i]);
    flag[i] = (i == 0 || cl == 4u || cl != ref_class (seq[i - 1])) ? 1u : 0u;
  }
}

__global__ void ref_seg_pos_kernel (const u32 *__restrict__ flag, const u32 *__restrict__ excl, long n, u32 *__restrict__ segpos)
{ // segpos[n_seg] = n closes the last segment
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    if (flag[i]) segpos[excl[i]] = (u32) i;
    if (i == n - 1) segpos[excl[i] + flag[i]] = (u32) n;
  }
}

// which segments become entries (a run of a base whose 2k flank bytes are all ACGTU: the delimiter is not, so both
// flanks lie in the run's contig) and which are delimiters.  Segments at and beyond *n_seg get zeros: the scans run over n.
__global__ void ref_seg_class_kernel (const uint8_t *__restrict__ seq, long n, int k, const u32 *__restrict__ segpos, const u32 *__restrict__ n_seg,
                                      u32 *__restrict__ vflag, u32 *__restrict__ nlflag)
{
  const long ns = (long) *n_seg;
  for (long j = blockIdx.x * (long) blockDim.x + threadIdx.x; j < n; j += (long) gridDim.x * blockDim.x) {
    u32 v = 0, nl = 0;
    if (j < ns) {
      const long s = segpos[j], e = (long) segpos[j + 1] - 1;
      const u32 b = seq[s];
      nl = b == '\n';
      if (byte_is_acgtu (b) && s - k >= 0 && e + k < n) {
        v = 1;
        for (int i = 1; i <= k; i++) if (!byte_is_acgtu (seq[s - i]) || !byte_is_acgtu (seq[e + i])) { v = 0; break; }
      }
    }
    vflag[j] = v; nlflag[j] = nl;
  }
}

__global__ void ref_nlpos_kernel (const u32 *__restrict__ segpos, const u32 *__restrict__ n_seg, const u32 *__restrict__ nlflag,
                                  const u32 *__restrict__ nlex, long n, u32 *__restrict__ nlpos)
{
  const long ns = (long) *n_seg;
  for (long j = blockIdx.x * (long) blockDim.x + threadIdx.x; j < ns && j < n; j += (long) gridDim.x * blockDim.x)
    if (nlflag[j]) nlpos[nlex[j]] = segpos[j];
}

// the entries in stream order, and the unsorted records of both orders (padded to n: the sort's size is fixed before the
// number of entries is known to the host)
__global__ void ref_entry_kernel (const uint8_t *__restrict__ seq, long n, int k, const u32 *__restrict__ segpos, const u32 *__restrict__ n_seg,
                                  const u32 *__restrict__ vflag, const u32 *__restrict__ vex, const u32 *__restrict__ n_ent,
                                  const u32 *__restrict__ nlex, const u32 *__restrict__ nlpos,
                                  RefEntry *__restrict__ entries, u64 *__restrict__ ord0, u64 *__restrict__ ord1)
{
  const long ns = (long) *n_seg, ne = (long) *n_ent;
  for (long j = blockIdx.x * (long) blockDim.x + threadIdx.x; j < n; j += (long) gridDim.x * blockDim.x) {
    if (j >= ne) {
      const u64 pad = LC_PAD_IDX << LC_IDX_SHIFT;
      ord0[3 * j] = 0; ord0[3 * j + 1] = 0; ord0[3 * j + 2] = pad;
      ord1[3 * j] = 0; ord1[3 * j + 1] = 0; ord1[3 * j + 2] = pad;
    }
    if (j >= ns || !vflag[j]) continue;
    const long s = segpos[j], e = (long) segpos[j + 1] - 1;
    u64 left = 0, right = 0;
    for (int i = 0; i < k; i++) {
      left |= (u64) byte_code (seq[s - k + i]) << (2 * i);
      right |= (u64) byte_code (seq[e + 1 + i]) << (2 * i);
    }
    u64 c0, c1; u32 base, flag;
    canonicalise (left, right, 0u, 0u, byte_code (seq[s]), k, c0, c1, base, flag);
    const long x = vex[j], ct = nlex[j], cstart = ct ? (long) nlpos[ct - 1] + 1 : 0;
    entries[x] = RefEntry {c0, c1, s - ct, (int) ct, (int) (s - cstart), (int) (e - s + 1), (int) base, flag == 2u ? 1 : 0, 0};
    const u64 word = (u64) base | ((u64) x << LC_IDX_SHIFT);
    ord0[3 * x] = c0; ord0[3 * x + 1] = c1; ord0[3 * x + 2] = word;
    ord1[3 * x] = c1; ord1[3 * x + 1] = c0; ord1[3 * x + 2] = word;
  }
}

extern "C" void tjamd_reference_destroy (tjamd_reference *ref)
{
  if (!ref) return;
  (void) hipSetDevice (ref->device);
  for (void *p : ref->owned) if (p) (void) hipFree (p);
  if (ref->seed) (void) hipFree (ref->seed);
  delete ref;
}

extern "C" tjamd_reference *tjamd_reference_create (tjamd_counter *c, const void *h_stream, size_t n_bytes)
{
  static const char *fn = "tjamd_reference_create";
  if (tjamd_device_count () <= 0) { set_err (TJAMD_ERR_NO_DEVICE, "%s: TJAMD_ERR_NO_DEVICE: no HIP device visible (the index is built on the device; no CPU fallback)", fn); return NULL; }
  if (!c) { set_err (TJAMD_ERR_ARG, "%s: null counter", fn); return NULL; }
  if (stream_refused (fn, h_stream, n_bytes)) return NULL;
  HIPCHK_NULL (hipSetDevice (c->device));
  Stage st (c, T_REF);
  std::unique_ptr<tjamd_reference, void (*) (tjamd_reference *)> ref (new tjamd_reference (), tjamd_reference_destroy);
  ref->device = c->device; ref->k = c->k;
  const long n = (long) n_bytes;
  if (n == 0) return ref.release ();
  ScratchCut cut;
  u32 *flag, *excl, *segpos, *nlflag, *nlex, *nlpos, *tot;
  cut.take (flag, n); cut.take (excl, n); cut.take (segpos, n + 1); cut.take (nlflag, n); cut.take (nlex, n); cut.take (nlpos, n + 1); cut.take (tot, 64);
  if (cut.commit (c) || upload_stream (c, fn, h_stream, n_bytes) || ensure (c->scan_tmp, scan_tmp_words (n) * 4 + 64, c->stream)) return NULL;
  for (int i = 0; i < 4; i++)
    if (hipMalloc (&ref->owned[i], (size_t) n * (i ? 24 : sizeof (RefEntry))) != hipSuccess) { set_err (TJAMD_ERR_HIP, "%s: hipMalloc failed for %ld bytes of genome", fn, n); return NULL; }
  u32 *n_seg = tot, *n_ent = tot + 1, *n_nl = tot + 2;
  const dim3 g (grid_for (n)), b (256);
  const uint8_t *seq = (const uint8_t *) c->stage.p;
  st.begin ();
  hipLaunchKernelGGL (ref_seg_flag_kernel, g, b, 0, c->stream, seq, n, flag);
  int rc = exclusive_scan (c, flag, excl, n, n_seg);
  hipLaunchKernelGGL (ref_seg_pos_kernel, g, b, 0, c->stream, (const u32 *) flag, (const u32 *) excl, n, segpos);
  u32 *vflag = flag, *vex = excl;                       // (both free again once the segment positions are written)
  hipLaunchKernelGGL (ref_seg_class_kernel, g, b, 0, c->stream, seq, n, c->k, (const u32 *) segpos, (const u32 *) n_seg, vflag, nlflag);
  if (!rc) rc = exclusive_scan (c, vflag, vex, n, n_ent);
  if (!rc) rc = exclusive_scan (c, nlflag, nlex, n, n_nl);
  hipLaunchKernelGGL (ref_nlpos_kernel, g, b, 0, c->stream, (const u32 *) segpos, (const u32 *) n_seg, (const u32 *) nlflag, (const u32 *) nlex, n, nlpos);
  u64 *r0 = (u64 *) ref->owned[1], *r1 = (u64 *) ref->owned[2], *r2 = (u64 *) ref->owned[3];
  hipLaunchKernelGGL (ref_entry_kernel, g, b, 0, c->stream, seq, n, c->k, (const u32 *) segpos, (const u32 *) n_seg, (const u32 *) vflag, (const u32 *) vex,
                      (const u32 *) n_ent, (const u32 *) nlex, (const u32 *) nlpos, (RefEntry *) ref->owned[0], r0, r1);
  if (rc || hipGetLastError () != hipSuccess) { if (!rc) set_err (TJAMD_ERR_HIP, "%s: launch failed", fn); return NULL; }
  if (radix_sort_records (c, r0, r2, n) || radix_sort_records (c, r1, r2, n)) return NULL;   // (results in r0 and r1, whichever blocks those now are)
  st.end ();
  u32 h[3] = {0, 0, 0};
  uint8_t last = 0;
  if (hipMemcpyAsync (h, tot, sizeof (h), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipMemcpyAsync (&last, seq + n - 1, 1, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize (c->stream) != hipSuccess) {
    set_err (TJAMD_ERR_HIP, "%s: build failed: %s", fn, hipGetErrorString (hipGetLastError ()));
    return NULL;
  }
  ref->entries = (RefEntry *) ref->owned[0]; ref->ord[0] = r0; ref->ord[1] = r1;
  ref->n_entries = (long) h[1]; ref->n_contigs = (long) h[2] + (last != '\n' ? 1 : 0);
  for (int i = 1; i < 4; i++) if (ref->owned[i] == (void *) r2) { (void) hipFree (r2); ref->owned[i] = nullptr; }   // the sort's spare block
  if (ref->n_entries < n) {                             // keep what the entries take, not what the stream could have held
    const size_t ne = (size_t) std::max<long> (ref->n_entries, 1);
    void *small[3] = {nullptr, nullptr, nullptr}, *big[3] = {ref->entries, ref->ord[0], ref->ord[1]};
    const size_t bytes[3] = {ne * sizeof (RefEntry), ne * 24, ne * 24};
    bool ok = true;
    for (int i = 0; i < 3 && ok; i++) ok = hipMalloc (&small[i], bytes[i]) == hipSuccess && hipMemcpy (small[i], big[i], bytes[i], hipMemcpyDeviceToDevice) == hipSuccess;
    if (ok) {
      for (void *&p : ref->owned) { if (p) (void) hipFree (p); p = nullptr; }
      for (int i = 0; i < 3; i++) ref->owned[i] = small[i];
      ref->entries = (RefEntry *) small[0]; ref->ord[0] = (u64 *) small[1]; ref->ord[1] = (u64 *) small[2];
    } else {                                            // (no room for the copies: the index stays in its first blocks)
      for (void *p : small) if (p) (void) hipFree (p);
      (void) hipGetLastError ();
    }
  }
  st.done ();
  return ref.release ();
}

extern "C" long tjamd_reference_entries (const tjamd_reference *ref) { return ref ? ref->n_entries : -1; }
extern "C" long tjamd_reference_contigs (const tjamd_reference *ref) { return ref ? ref->n_contigs : -1; }
extern "C" long tjamd_reference_download (const tjamd_reference *ref, tjamd_ref_entry *out, long capacity)
{
  if (!ref || (ref->n_entries && !out)) return -set_err (TJAMD_ERR_ARG, "tjamd_reference_download: null reference or buffer");
  if (ref->n_entries > capacity) return -set_err (TJAMD_ERR_CAPACITY, "tjamd_reference_download: %ld entries, caller capacity %ld", ref->n_entries, capacity);
  if (ref->n_entries && (hipSetDevice (ref->device) != hipSuccess || hipMemcpy (out, ref->entries, (size_t) ref->n_entries * sizeof (RefEntry), hipMemcpyDeviceToHost) != hipSuccess))
    return -set_err (TJAMD_ERR_HIP, "tjamd_reference_download: copy failed");
  return ref->n_entries;
}
TJ_LAST_MS (tjamd_last_reference_ms, T_REF)

// ---- the lookup --------------------------------------------------------------------------------------------------
// Thread mapping: a lane per query finds its two buckets (the entries with its base and its exact flank) by binary search
// and walks a bucket of up to LC_LANE_WALK entries by itself: at k >= 12 nearly every bucket has 0 to 2 entries and the 64
// lanes stay in step.  A longer bucket (thousands of entries at k = 5) is handed to the whole wavefront: the owner's query
// and bounds are broadcast, the 64 lanes read the bucket as contiguous records and the result is reduced with shuffles, so
// the time of a wavefront is the sum of its long buckets over 64, not the longest one times 64.

#define LC_LANE_WALK 16

// The host path of both lookups behind their argument checks and the counter's device: the interval of `slot`, nothing to do for
// no row, the count word cleared, the lookup's launch (which gets the word), the count read back and returned
template <class Launch> static long lookup_rows (tjamd_counter *c, const char *fn, int slot, long n, Launch &&launch)
{
  Stage st (c, slot);
  if (n == 0) return 0;
  u32 *n_located, found = 0;
  int rc = flags_alone (c, fn, n_located);
  if (rc) return -rc;
  st.begin ();
  launch (n_located);
  st.end ();
  rc = read_back (c, fn, n_located, &found, 1);
  if (rc) return -rc;
  st.done ();
  return (long) found;
}

// first record of ord[0, n) (descending by base, primary) that does not sort before / that sorts behind (base, primary)
__device__ __forceinline__ long ord_bound (const u64 *__restrict__ ord, long n, u32 qb, u64 qp, bool behind)
{
  long lo = 0, hi = n;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    const u64 p = ord[3 * mid];
    const u32 b = (u32) ord[3 * mid + 2] & 3u;
    const bool before = b > qb || (b == qb && (behind ? p >= qp : p > qp));
    if (before) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The range walk of both lookups, the mapping above, called by all 64 lanes: a lane's own range [lo, hi) and its NQ query words q;
// try_record (i, q, best, hits) is the lookup's step for record i.  Of a long range the bounds and q are broadcast from its owner,
// (best, hits) is reduced with shuffles and folded into the owner's.
template <int NQ, class Try>
__device__ __forceinline__ void lc_walk_range (int lane, long lo, long hi, const u64 (&q)[NQ], u64 &best, u32 &hits, Try try_record)
{
  const bool mine = hi - lo <= LC_LANE_WALK;
  if (mine) for (long i = lo; i < hi; i++) try_record (i, q, best, hits);
  u64 big = __ballot (!mine);
  while (big) {                                         // the wavefront walks its long ranges together, one after the other
    const int src = __ffsll ((long long) big) - 1;
    big &= big - 1;
    const long blo = __shfl (lo, src), bhi = __shfl (hi, src);
    u64 bq[NQ];
#pragma unroll
    for (int w = 0; w < NQ; w++) bq[w] = __shfl (q[w], src);
    u64 wb = ~0ull; u32 wh = 0;
    for (long i = blo + lane; i < bhi; i += 64) try_record (i, bq, wb, wh);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const u64 ob = __shfl_xor (wb, o); wb = ob < wb ? ob : wb; wh += __shfl_xor (wh, o); }
    if (lane == src) { best = wb < best ? wb : best; hits += wh; }
  }
}

// one record against a query's inexact flank: best = (mismatches << 32 | entry number), the smallest wins
__device__ __forceinline__ void locate_try (const u64 *__restrict__ ord, long i, u64 qs, int maxm, bool skip_exact, u64 &best, u32 &hits)
{
  const int d = flank_hamming (ord[3 * i + 1], qs);
  if (d <= maxm && !(skip_exact && d == 0)) {           // (exact in both flanks: counted on the ctx0 side)
    hits++;
    const u64 cand = ((u64) d << 32) | ((ord[3 * i + 2] >> LC_IDX_SHIFT) & 0xFFFFFFFFull);
    best = cand < best ? cand : best;
  }
}

__global__ __launch_bounds__ (256)
void locate_kernel (const u64 *__restrict__ keys, long n, const u64 *__restrict__ ord0, const u64 *__restrict__ ord1, long n_ent,
                    const RefEntry *__restrict__ entries, int maxm, Location *__restrict__ loc, u32 *__restrict__ n_located)
{
  const int lane = threadIdx.x & 63;
  const long stride = (long) gridDim.x * blockDim.x;
  for (long q0 = blockIdx.x * (long) blockDim.x + (threadIdx.x & ~63); q0 < n; q0 += stride) {     // (uniform across a wavefront)
    const long q = q0 + lane;
    const bool active = q < n;
    u64 qc[2] = {0, 0}; u32 qb = 0;
    if (active) { qc[0] = keys[3 * q]; qc[1] = keys[3 * q + 1]; qb = (u32) keys[3 * q + 2] & 3u; }
    u64 best = ~0ull; u32 hits = 0;
#pragma unroll
    for (int side = 0; side < 2; side++) {
      const u64 *__restrict__ ord = side ? ord1 : ord0;
      const u64 qp = qc[side], qs[1] = {qc[1 - side]};
      long lo = 0, hi = 0;
      if (active) { lo = ord_bound (ord, n_ent, qb, qp, false); hi = ord_bound (ord, n_ent, qb, qp, true); }
      lc_walk_range (lane, lo, hi, qs, best, hits, [&] (long i, const u64 (&q)[1], u64 &b, u32 &h) { locate_try (ord, i, q[0], maxm, side == 1, b, h); });
    }
    Location o = LC_NOWHERE;
    if (hits) {
      const RefEntry e = entries[best & 0xFFFFFFFFull];
      o = Location {e.flat, e.contig, e.pos, e.length, (int) (best >> 32), e.neg_strand, (int) hits};
    }
    if (active) loc[q] = o;
    const u64 found = __ballot (active && hits);
    if (lane == 0 && found) atomicAdd (n_located, (u32) __popcll (found));
  }
}

extern "C" long tjamd_locate (tjamd_counter *c, const tjamd_reference *ref, const void *d_keys, long n, int max_mismatches, tjamd_location *d_loc)
{
  static const char *fn = "tjamd_locate";
  if (!c || !ref) return -set_err (TJAMD_ERR_ARG, "%s: null counter or reference", fn);
  if (const int bad = reference_of_counter (fn, ref, c)) return -bad;
  if (max_mismatches < 0 || max_mismatches > c->k) return -set_err (TJAMD_ERR_ARG, "%s: max_mismatches %d outside 0..%d", fn, max_mismatches, c->k);
  if (n < 0) return -set_err (TJAMD_ERR_ARG, "%s: n %ld < 0", fn, n);
  if (n >= (1l << 31)) return -set_err (TJAMD_ERR_CAPACITY, "%s: %ld rows", fn, n);
  if (n > 0 && (!d_keys || !d_loc)) return -set_err (TJAMD_ERR_ARG, "%s: null key or location buffer", fn);
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  return lookup_rows (c, fn, T_LOCATE, n, [&] (u32 *n_located) {
    hipLaunchKernelGGL (locate_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const u64 *) d_keys, n, (const u64 *) ref->ord[0], (const u64 *) ref->ord[1],
                        ref->n_entries, (const RefEntry *) ref->entries, max_mismatches, (Location *) d_loc, n_located);
  });
}
TJ_LAST_MS (tjamd_last_locate_ms, T_LOCATE)

// ---- N10: the second pass of the lookup: flanks that differ from the genome by indels, or in both flanks -----------------
// The reference maps context + tract with BWA, by edit distance over the whole string (src/hopo_counter.c:495-572), and allows
// shifts of up to three bases per flank when it rescans (distance_between_context_kmer_pair_with_edit_shift, :81-113).
// Here: a banded unit-cost edit distance per flank, anchored at the tract and free at the outer end, on the entries that
// share the inner half of one flank with the row (the seed).  include/tatajuba_locate.h has the rule, DESIGN.md section 3.5,
// N10, the order, the mapping and the measurements.

#define LG_MAX_SHIFT TJAMD_MAX_SHIFT
#define LG_INF       1000

__host__ __device__ __forceinline__ u64 flank_mask (int k) { return (k >= 32) ? ~0ull : ((1ull << (2 * k)) - 1ull); }   // (no shift by 64)

// the k bases of a packed flank in reverse order (no complement): base i goes to base k - 1 - i.  1 <= k <= 32.
__host__ __device__ __forceinline__ u64 rev_k (u64 x, int k)
{
  x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
  x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
  return __builtin_bswap64 (x) >> (64 - 2 * k);
}

// d_B (q, r) of two inner-first flanks (inner base i at bits 2i, nothing above base k - 1): row i of the band holds
// D[i][i - B ... i + B] in 2B + 1 registers (cell t is column j = i + t - B; every index below is a compile-time number once
// the loops over t are unrolled).  win holds r[i - 1 - B ... i - 1 + B], the bases row i compares q[i - 1] with, base t at bits
// 2t; it moves on by one base per row, so no shift reaches 64 bits at k = 32.  Columns beyond k only feed columns beyond k
// and are left out at the end; columns below 0 are LG_INF.
template <int B>
__host__ __device__ __forceinline__ int flank_edit_distance (u64 q, u64 r, int k)
{
  constexpr int W = 2 * B + 1;
  int prev[W], cur[W];
#pragma unroll
  for (int t = 0; t < W; t++) prev[t] = t >= B ? t - B : LG_INF;        // D[0][j] = j
  u64 win = (r << (2 * B)) & ((1ull << (2 * W)) - 1ull);
  int col = k <= B ? k : LG_INF;                                        // the last column, D[i][k] for i >= k - B: D[0][k] = k
  for (int i = 1; i <= k; i++) {
    const u32 qi = (u32) q & 3u;
    q >>= 2;
#pragma unroll
    for (int t = 0; t < W; t++) {
      const int j = i + t - B;
      int v = prev[t] + (((u32) (win >> (2 * t)) & 3u) != qi ? 1 : 0);
      if (t + 1 < W) v = min (v, prev[t + 1] + 1);
      if (t > 0) v = min (v, cur[t - 1] + 1);
      v = j < 0 ? LG_INF : (j == 0 ? i : v);
      cur[t] = v;
      col = j == k ? min (col, v) : col;
    }
#pragma unroll
    for (int t = 0; t < W; t++) prev[t] = cur[t];
    const int nb = i + B;                                               // the base that enters the window for row i + 1
    win = (win >> 2) | ((nb < k ? (r >> (2 * nb)) & 3ull : 0ull) << (4 * B));
  }
  int best = col;                                                       // the last row: D[k][k - B ... k]
#pragma unroll
  for (int t = 0; t <= B; t++) best = min (best, prev[t]);
  return best;
}

// the same for a caller on the host: the packed flanks as the index and the union rows hold them (side 0: ctx0, inner base
// at the high end; side 1: ctx1, inner base at bit 0).  No device call: a CPU test runs the kernel's own arithmetic.
extern "C" int tjamd_flank_edit_distance (uint64_t a, uint64_t b, int k, int side, int max_shift)
{
  static const char *fn = "tjamd_flank_edit_distance";
  if (k < 1 || k > 32) return -set_err (TJAMD_ERR_ARG, "%s: k %d outside 1..32", fn, k);
  if (side < 0 || side > 1) return -set_err (TJAMD_ERR_ARG, "%s: side %d outside 0..1", fn, side);
  if (max_shift < 0 || max_shift > LG_MAX_SHIFT) return -set_err (TJAMD_ERR_ARG, "%s: max_shift %d outside 0..%d", fn, max_shift, LG_MAX_SHIFT);
  u64 q = a & flank_mask (k), r = b & flank_mask (k);
  if (side == 0) { q = rev_k (q, k); r = rev_k (r, k); }
  switch (max_shift) {
    case 0: return flank_edit_distance<0> (q, r, k);
    case 1: return flank_edit_distance<1> (q, r, k);
    case 2: return flank_edit_distance<2> (q, r, k);
    default: return flank_edit_distance<3> (q, r, k);
  }
}

// the unsorted records of the third order: (rev_k (ctx1), ctx0, word) -- the inner bases of ctx1 are its low bits, reversed
// they are the high bits, and the entries that share them with a row are a contiguous range, as those of ctx0 are in ord[0]
__global__ void ref_seed_kernel (const RefEntry *__restrict__ entries, long n, int k, u64 *__restrict__ rec)
{
  for (long x = blockIdx.x * (long) blockDim.x + threadIdx.x; x < n; x += (long) gridDim.x * blockDim.x) {
    const u64 c0 = entries[x].ctx0, c1 = entries[x].ctx1;
    rec[3 * x] = rev_k (c1, k); rec[3 * x + 1] = c0; rec[3 * x + 2] = (u64) (u32) entries[x].base | ((u64) x << LC_IDX_SHIFT);
  }
}

extern "C" int tjamd_reference_has_seeds (const tjamd_reference *ref) { return ref && ref->has_seeds ? 1 : 0; }

extern "C" long tjamd_reference_add_seeds (tjamd_counter *c, tjamd_reference *ref)
{
  static const char *fn = "tjamd_reference_add_seeds";
  if (!c || !ref) return -set_err (TJAMD_ERR_ARG, "%s: null counter or reference", fn);
  if (const int bad = reference_of_counter (fn, ref, c)) return -bad;
  if (ref->has_seeds) return ref->n_entries;
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  Stage st (c, T_SEED_ORDER);
  const long n = ref->n_entries;
  if (n == 0) { ref->has_seeds = true; return 0; }
  const size_t bytes = (size_t) n * 24;
  int rc = ensure (c->lc_work, bytes, c->stream);           // the sort's spare block
  if (rc) return -rc;
  void *block = nullptr;
  if (hipMalloc (&block, bytes) != hipSuccess) { (void) hipGetLastError (); return -set_err (TJAMD_ERR_HIP, "%s: hipMalloc failed for %ld entries", fn, n); }
  // the sort swaps its two blocks once per pass: start in the one that leaves the result in the reference's own
  u64 *a = (key_passes (c->k) & 1) ? (u64 *) c->lc_work.p : (u64 *) block, *b = (key_passes (c->k) & 1) ? (u64 *) block : (u64 *) c->lc_work.p;
  st.begin ();
  hipLaunchKernelGGL (ref_seed_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const RefEntry *) ref->entries, n, c->k, a);
  if (hipGetLastError () != hipSuccess) { (void) hipFree (block); return -set_err (TJAMD_ERR_HIP, "%s: launch failed", fn); }
  rc = radix_sort_records (c, a, b, n);
  if (rc) { (void) hipStreamSynchronize (c->stream); (void) hipFree (block); return -rc; }
  st.end ();
  rc = read_back (c, fn, nullptr, nullptr, 0);
  if (rc) { (void) hipFree (block); return -rc; }
  if (a != (u64 *) block) {                                // (the parity of key_passes chose the starting block: cannot happen)
    (void) hipFree (block);
    return -set_err (TJAMD_ERR_STATE, "%s: the sorted order did not end in the reference's block after %d passes", fn, key_passes (c->k));
  }
  ref->seed = (u64 *) block; ref->has_seeds = true;
  st.done ();
  return n;
}
TJ_LAST_MS (tjamd_last_seed_order_ms, T_SEED_ORDER)

// ---- the gapped lookup ---------------------------------------------------------------------------------------------
// Thread mapping: that of locate_kernel, for its reason (at k >= 12 nearly every range is short and the 64 lanes stay in
// step; a long range costs its length over 64).  The two ranges of a row are the entries with its base and the inner h
// bases of its ctx0 (in ord[0]) or of its ctx1 (in the seed order).  A lane runs both banded distances on each candidate;
// 64 lanes on 64 candidates run the same k rows of the same band.

// one record of order `side` against a row: both flanks inner-first (q0, q1: the row's; seed_mask: the inner h bases).
// An entry that shares the row's ctx0 seed is counted in ord[0] only.  best = (edits << 32 | entry number), the smallest wins.
template <int B>
__device__ __forceinline__ void gapped_try (const u64 *__restrict__ ord, long i, int side, int k, u64 q0, u64 q1, u64 seed_mask, int max_edits, u64 &best, u32 &hits)
{
  const u64 p = ord[3 * i], s = ord[3 * i + 1];
  const u64 r0 = rev_k (side ? s : p, k), r1 = side ? rev_k (p, k) : s;
  if (side && ((r0 ^ q0) & seed_mask) == 0ull) return;
  const int d = flank_edit_distance<B> (q0, r0, k) + flank_edit_distance<B> (q1, r1, k);
  if (d <= max_edits) {
    hits++;
    const u64 cand = ((u64) d << 32) | ((ord[3 * i + 2] >> LC_IDX_SHIFT) & 0xFFFFFFFFull);
    best = cand < best ? cand : best;
  }
}

template <int B>
__global__ __launch_bounds__ (256)
void locate_gapped_kernel (const u64 *__restrict__ keys, long n, const u64 *__restrict__ ord0, const u64 *__restrict__ ords, long n_ent,
                           const RefEntry *__restrict__ entries, int k, int max_edits, Location *loc, int *__restrict__ how, u32 *__restrict__ n_located)
{
  const int lane = threadIdx.x & 63;
  const long stride = (long) gridDim.x * blockDim.x;
  const int h = (k + 1) / 2, sh = 2 * (k - h);                          // (sh <= 32)
  const u64 seed_mask = flank_mask (h), rest = (1ull << sh) - 1ull;
  for (long q0 = blockIdx.x * (long) blockDim.x + (threadIdx.x & ~63); q0 < n; q0 += stride) {     // (uniform across a wavefront)
    const long q = q0 + lane;
    const bool active = q < n;
    const bool todo = active && loc[q].flat < 0;                        // (a located row skips the searches, not the hand-offs)
    u64 qc0 = 0, qc1 = 0; u32 qb = 0;
    if (todo) { qc0 = keys[3 * q]; qc1 = keys[3 * q + 1]; qb = (u32) keys[3 * q + 2] & 3u; }
    const u64 qi[2] = {rev_k (qc0, k), qc1};                            // inner-first
    u64 best = ~0ull; u32 hits = 0;
#pragma unroll
    for (int side = 0; side < 2; side++) {
      const u64 *__restrict__ ord = side ? ords : ord0;
      const u64 top = (side ? rev_k (qc1, k) : qc0) | rest, bottom = top & ~rest;     // every primary flank with the row's inner h bases
      long lo = 0, hi = 0;
      if (todo) { lo = ord_bound (ord, n_ent, qb, top, false); hi = ord_bound (ord, n_ent, qb, bottom, true); }
      lc_walk_range (lane, lo, hi, qi, best, hits, [&] (long i, const u64 (&q)[2], u64 &b, u32 &h) { gapped_try<B> (ord, i, side, k, q[0], q[1], seed_mask, max_edits, b, h); });
    }
    if (todo && hits) {
      const RefEntry e = entries[best & 0xFFFFFFFFull];
      loc[q] = Location {e.flat, e.contig, e.pos, e.length, (int) (best >> 32), e.neg_strand, (int) hits};
    }
    if (active && how) how[q] = !todo ? 0 : (hits ? 1 : -1);
    const u64 found = __ballot (todo && hits);
    if (lane == 0 && found) atomicAdd (n_located, (u32) __popcll (found));
  }
}

extern "C" long tjamd_locate_gapped (tjamd_counter *c, const tjamd_reference *ref, const void *d_keys, long n, int max_edits, int max_shift,
                                     tjamd_location *d_loc, int *d_how)
{
  static const char *fn = "tjamd_locate_gapped";
  // (what can be refused without reading the counter or the reference comes first)
  if (!c || !ref) return -set_err (TJAMD_ERR_ARG, "%s: null counter or reference", fn);
  if (max_shift < 0 || max_shift > LG_MAX_SHIFT) return -set_err (TJAMD_ERR_ARG, "%s: max_shift %d outside 0..%d", fn, max_shift, LG_MAX_SHIFT);
  if (max_edits < 0) return -set_err (TJAMD_ERR_ARG, "%s: max_edits %d outside 0..k", fn, max_edits);
  if (n < 0) return -set_err (TJAMD_ERR_ARG, "%s: n %ld < 0", fn, n);
  if (n >= (1l << 31)) return -set_err (TJAMD_ERR_CAPACITY, "%s: %ld rows", fn, n);
  if (n > 0 && (!d_keys || !d_loc)) return -set_err (TJAMD_ERR_ARG, "%s: null key or location buffer", fn);
  if (const int bad = reference_of_counter (fn, ref, c)) return -bad;
  if (!ref->has_seeds) return -set_err (TJAMD_ERR_ARG, "%s: the reference has no seed order (tjamd_reference_add_seeds comes first)", fn);
  if (max_edits > c->k) return -set_err (TJAMD_ERR_ARG, "%s: max_edits %d outside 0..%d", fn, max_edits, c->k);
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  return lookup_rows (c, fn, T_LOCATE_GAPPED, n, [&] (u32 *n_located) {
#define LG_LAUNCH(B) hipLaunchKernelGGL (locate_gapped_kernel<B>, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const u64 *) d_keys, n, (const u64 *) ref->ord[0], \
                                           (const u64 *) ref->seed, ref->n_entries, (const RefEntry *) ref->entries, c->k, max_edits, (Location *) d_loc, d_how, n_located)
    switch (max_shift) { case 0: LG_LAUNCH (0); break; case 1: LG_LAUNCH (1); break; case 2: LG_LAUNCH (2); break; default: LG_LAUNCH (3); break; }
#undef LG_LAUNCH
  });
}
TJ_LAST_MS (tjamd_last_locate_gapped_ms, T_LOCATE_GAPPED)

// ---- tracts by location ------------------------------------------------------------------------------------------

// the context-keyed tracts of tjamd_tract_ids as tjamd_union_tract (for a caller that passes no tracts): one thread per head
__global__ void lt_context_tract_kernel (long n, const long long *__restrict__ total, const u32 *__restrict__ head, const u32 *__restrict__ excl,
                                         UnionTract *__restrict__ tracts)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    if (i > 0 && !head[i]) continue;
    UnionTract o = {(int) i, 0, 1, (int) i, 0, 0, 0};
    long long mode_count = 0;
    for (long j = i; j < n && (j == i || !head[j]); j++) {
      const long long cj = total[j];
      if (j == i || mode_count < cj) { mode_count = cj; o.mode = (int) j; }
      o.integral += cj; o.n_rows++;
    }
    tracts[excl[i] + head[i]] = o;
  }
}

#define LT_KEY_PASSES 6                 // 48 bits of key:
#define LT_FLAT_MAX   (1ll << 45)       // (flat + 1) << 2 | base stays below 2^48 for flat below 2^45; larger ones are refused

// a tract's sort key: 0 if it has no located row, else (flat + 1) << 2 | base of its located row with the highest total
// (the first of equal totals).  Also checks that the tracts tile the union (err = 1 where breaks_tiling says so).
__global__ void lt_tract_key_kernel (const UnionTract *__restrict__ tracts, long nt, long n, const u64 *__restrict__ keys, const long long *__restrict__ total,
                                     const Location *__restrict__ loc, u64 *__restrict__ key, u32 *__restrict__ val, int *__restrict__ err)
{
  for (long t = blockIdx.x * (long) blockDim.x + threadIdx.x; t < nt; t += (long) gridDim.x * blockDim.x) {
    const long first = tracts[t].first, rows = tracts[t].n_rows;
    u64 kk = 0;
    if (breaks_tiling (tracts, nt, n, t)) *err = 1;
    else {
      long best = -1; long long best_total = 0;
      for (long r = first; r < first + rows; r++)
        if (loc[r].flat >= 0 && (best < 0 || total[r] > best_total)) { best = r; best_total = total[r]; }
      if (best >= 0 && loc[best].flat >= LT_FLAT_MAX) *err = 2;   // (the sort below would drop its upper bits)
      else if (best >= 0) kk = ((u64) (loc[best].flat + 1) << 2) | (keys[3 * first + 2] & 3ull);
    }
    key[t] = kk; val[t] = (u32) t;
  }
}

// stable ascending LSD radix sort of (64-bit key, 32-bit value) pairs, a digit of 8 bits per pass: the count / scatter
// pair of radix_count_kernel / radix_scatter_kernel for keys that are not records
__global__ __launch_bounds__ (256)
void kv_count_kernel (const u64 *__restrict__ key, long n, int pass, u32 *__restrict__ hist, int nblk)
{
  __shared__ u32 h[256];
  const int tid = threadIdx.x, lane = tid & 63;
  const u64 lt = (1ull << lane) - 1ull;
  h[tid] = 0;
  __syncthreads ();
  const long base = (long) blockIdx.x * RS_ITEMS;
  for (int i = tid; i < RS_ITEMS; i += 256) {
    const long r = base + i;
    const bool active = r < n;
    const u32 d = active ? (u32) (key[r] >> (8 * pass)) & 0xFFu : 0u;
    const u64 peers = match_digit (d, active);
    if (active && (peers & lt) == 0ull) atomicAdd (&h[d], (u32) __popcll (peers));
  }
  __syncthreads ();
  hist[(long) tid * nblk + blockIdx.x] = h[tid];
}

__global__ __launch_bounds__ (256)
void kv_scatter_kernel (const u64 *__restrict__ key, const u32 *__restrict__ val, u64 *__restrict__ key_out, u32 *__restrict__ val_out, long n, int pass,
                        const u32 *__restrict__ offs, int nblk)
{
  __shared__ u32 wcnt[4][256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < 1024; i += 256) (&wcnt[0][0])[i] = 0;
  __syncthreads ();
  const long wbase = (long) blockIdx.x * RS_ITEMS + (long) wave * RS_WAVE_ITEMS;
  const u64 lt = (1ull << lane) - 1ull;
  for (int r = 0; r < RS_WAVE_ITEMS / 64; r++) {
    const long idx = wbase + r * 64 + lane;
    const bool active = idx < n;
    const u32 d = active ? (u32) (key[idx] >> (8 * pass)) & 0xFFu : 0u;
    const u64 peers = match_digit (d, active);
    if (active && (peers & lt) == 0ull) atomicAdd (&wcnt[wave][d], (u32) __popcll (peers));
  }
  __syncthreads ();
  {
    u32 run = offs[(long) tid * nblk + blockIdx.x];
    for (int w = 0; w < 4; w++) { u32 cnt = wcnt[w][tid]; wcnt[w][tid] = run; run += cnt; }
  }
  __syncthreads ();
  for (int r = 0; r < RS_WAVE_ITEMS / 64; r++) {
    const long idx = wbase + r * 64 + lane;
    const bool active = idx < n;
    u64 kk = 0; u32 v = 0, d = 0;
    if (active) { kk = key[idx]; v = val[idx]; d = (u32) (kk >> (8 * pass)) & 0xFFu; }
    const u64 peers = match_digit (d, active);
    const int leader = active ? (__ffsll ((long long) peers) - 1) : 0;
    u32 old = 0;
    if (active && lane == leader) old = atomicAdd (&wcnt[wave][d], (u32) __popcll (peers));
    old = __shfl (old, leader);
    if (active) { const u64 at = (u64) old + (u64) __popcll (peers & lt); key_out[at] = kk; val_out[at] = v; }
  }
}

// scratch of kv_sort for up to n_sort pairs: the blocks' histograms, and room in c->scan_tmp for their scan and for the
// caller's own scans of up to n_scan words (then 64 bytes).  Called before a stage begins: growing a buffer waits for the stream.
static int reserve_sort (tjamd_counter *c, long n_sort, long n_scan)
{
  const long nh = 256l * ((n_sort + RS_ITEMS - 1) / RS_ITEMS);
  const int rc = ensure (c->hist, (size_t) nh * 4, c->stream);
  return rc ? rc : ensure (c->scan_tmp, std::max (scan_tmp_words (nh), scan_tmp_words (n_scan)) * 4 + 64, c->stream);
}

// Queues the sort of the n pairs (key[0][i], val[0][i]) on the low `bits` of the key, ascending and stable: one pass per
// 8 bits between the two halves, whose pointers are swapped so that the result is in key[0] and val[0] again.
static int kv_sort (tjamd_counter *c, u64 *(&key)[2], u32 *(&val)[2], long n, int bits)
{
  const int nblk = (int) ((n + RS_ITEMS - 1) / RS_ITEMS);
  for (int p = 0; p < (bits + 7) / 8; p++) {
    hipLaunchKernelGGL (kv_count_kernel, dim3 (nblk), dim3 (256), 0, c->stream, (const u64 *) key[0], n, p, (u32 *) c->hist.p, nblk);
    const int rc = exclusive_scan (c, (const u32 *) c->hist.p, (u32 *) c->hist.p, 256l * nblk, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL (kv_scatter_kernel, dim3 (nblk), dim3 (256), 0, c->stream, (const u64 *) key[0], (const u32 *) val[0], key[1], val[1], n, p,
                        (const u32 *) c->hist.p, nblk);
    std::swap (key[0], key[1]); std::swap (val[0], val[1]);
  }
  return TJAMD_OK;
}


// the sorted tracts: where a merged tract starts (a new key, or no location: every unlocated tract stays alone) and the
// rows each brings
__global__ void lt_head_kernel (const u64 *__restrict__ key, const u32 *__restrict__ val, long nt, const UnionTract *__restrict__ tracts,
                                u32 *__restrict__ head, u32 *__restrict__ rows)
{
  for (long j = blockIdx.x * (long) blockDim.x + threadIdx.x; j < nt; j += (long) gridDim.x * blockDim.x) {
    head[j] = (j == 0 || key[j] == 0ull || key[j] != key[j - 1]) ? 1u : 0u;
    rows[j] = (u32) max (tracts[val[j]].n_rows, 0);
  }
}

// output row i is input row perm[i]: the sorted tract whose rows cover i (rowstart: exclusive scan of rows), its rows in union order
__global__ void lt_perm_kernel (long n, long nt, const u32 *__restrict__ rowstart, const u32 *__restrict__ val, const UnionTract *__restrict__ tracts,
                                const u64 *__restrict__ keys, int *__restrict__ perm, u64 *__restrict__ out_keys)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    long lo = 0, hi = nt;                               // last j with rowstart[j] <= i
    while (hi - lo > 1) { const long mid = (lo + hi) >> 1; if ((long) rowstart[mid] <= i) lo = mid; else hi = mid; }
    long r = (long) tracts[val[lo]].first + (i - (long) rowstart[lo]);
    if (r < 0 || r >= n) r = 0;                         // (tracts that do not tile the union: refused at the end of the call)
    perm[i] = (int) r;
    if (out_keys) { out_keys[3 * i] = keys[3 * r]; out_keys[3 * i + 1] = keys[3 * r + 1]; out_keys[3 * i + 2] = keys[3 * r + 2]; }
  }
}

__global__ void lt_gather_counts_kernel (const int *__restrict__ counts, const int *__restrict__ perm, long n, int ns, int *__restrict__ out)
{
  const long total = n * (long) ns;
  for (long x = blockIdx.x * (long) blockDim.x + threadIdx.x; x < total; x += (long) gridDim.x * blockDim.x) {
    const long i = x / ns; const int s = (int) (x - i * ns);
    out[x] = counts[(long) perm[i] * ns + s];
  }
}

// one thread per merged tract (at its first member): sums, flags, the modal output row, and the location of its located
// row with the highest total (the first in output order on a tie: that of its first member's, all members sharing flat)
__global__ void lt_merge_kernel (long nt, long n, const u32 *__restrict__ head, const u32 *__restrict__ hex, const u32 *__restrict__ rowstart,
                                 const u32 *__restrict__ val, const UnionTract *__restrict__ tracts, const long long *__restrict__ total,
                                 const Location *__restrict__ loc, long cap, UnionTract *__restrict__ out, Location *__restrict__ out_loc, int *__restrict__ ref_length)
{
  for (long j = blockIdx.x * (long) blockDim.x + threadIdx.x; j < nt; j += (long) gridDim.x * blockDim.x) {
    if (!head[j]) continue;
    const long g = hex[j];
    if (g >= cap) continue;
    UnionTract o = {(int) rowstart[j], 0, 0, (int) rowstart[j], 0, 0, 0};
    long long mode_total = 0, loc_total = 0; long loc_row = -1; bool have_mode = false;
    for (long m = j; m < nt && (m == j || !head[m]); m++) {
      const UnionTract t = tracts[val[m]];
      o.n_rows += t.n_rows; o.n_context += t.n_context; o.integral += t.integral; o.indel |= t.indel; o.lev_distance = max (o.lev_distance, t.lev_distance);
      for (long x = 0; x < t.n_rows; x++) {
        const long r = (long) t.first + x;
        if (r < 0 || r >= n) break;
        const long long tr = total[r];
        if (!have_mode || tr > mode_total) { have_mode = true; mode_total = tr; o.mode = (int) ((long) rowstart[m] + x); }
        if (loc[r].flat >= 0 && (loc_row < 0 || tr > loc_total)) { loc_row = r; loc_total = tr; }
      }
    }
    out[g] = o;
    const Location l = loc_row >= 0 ? loc[loc_row] : LC_NOWHERE;
    if (out_loc) out_loc[g] = l;
    if (ref_length) ref_length[g] = l.ref_length;
  }
}

extern "C" long tjamd_located_tracts (tjamd_counter *c, const void *d_keys, const void *d_counts, long n_union, int n_samples,
                                      const tjamd_union_tract *d_tracts, long n_tracts, const tjamd_location *d_loc,
                                      int *d_perm, void *d_out_keys, void *d_out_counts,
                                      tjamd_union_tract *d_out_tracts, tjamd_location *d_tract_loc, int *d_ref_length, long capacity)
{
  static const char *fn = "tjamd_located_tracts";
  int rc = union_args (fn, d_keys, d_counts, n_union, n_samples);
  if (rc) return -rc;
  if (n_union > 0 && (!d_loc || !d_perm || !d_out_tracts)) return -set_err (TJAMD_ERR_ARG, "%s: null location, permutation or tract buffer", fn);
  if (d_tracts && (rc = tract_count_arg (fn, n_tracts, n_union))) return -rc;   // (no tracts: the context-keyed ones, n_tracts unread)
  if (capacity < (n_union > 0 ? 1 : 0)) return -set_err (TJAMD_ERR_CAPACITY, "%s: capacity %ld for a union of %ld rows", fn, capacity, n_union);
  if (!c) return -set_err (TJAMD_ERR_ARG, "%s: null counter", fn);
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  Stage st (c, T_LOCATED_TRACTS);
  const long n = n_union;
  if (n == 0) return 0;
  ScratchCut cut;
  UnionTract *own; u64 *key[2]; u32 *val[2], *head, *hex, *rows, *rowstart, *tot;
  cut.take (own, n); cut.take (key[0], n); cut.take (key[1], n); cut.take (val[0], n); cut.take (val[1], n);
  cut.take (head, n); cut.take (hex, n); cut.take (rows, n); cut.take (rowstart, n); cut.take (tot, 64);
  rc = cut.commit (c);
  if (!rc) rc = ensure (c->ut_tot, (size_t) n * 8, c->stream);
  if (!rc) rc = reserve_sort (c, n, n);                 // (sized before the number of tracts is known: at most one per row)
  if (rc) return -rc;
  long long *total = (long long *) c->ut_tot.p;
  u32 *n_out = tot; int *err = (int *) tot + 1;
  if (hipMemsetAsync (tot, 0, 256, c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: memset failed", fn);
  st.begin ();
  const int S = tract_segment (n_samples);
  hipLaunchKernelGGL (union_totals_kernel, dim3 (tract_grid (n, S)), dim3 (256), 0, c->stream, (const int *) d_counts, n, n_samples, S, total);
  const UnionTract *tracts = (const UnionTract *) d_tracts;
  long nt = n_tracts;
  if (!tracts) {                                        // the context-keyed tracts: their number is needed on the host (one wait more)
    hipLaunchKernelGGL (tract_head_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const u64 *) d_keys, n, head);
    rc = exclusive_scan (c, head, hex, n, tot + 2);
    if (rc) return -rc;
    hipLaunchKernelGGL (lt_context_tract_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, n, (const long long *) total, (const u32 *) head, (const u32 *) hex, own);
    u32 nh = 0;
    rc = read_back (c, fn, tot + 2, &nh, 1);
    if (rc) return -rc;
    tracts = own; nt = (long) nh + 1;
  }
  hipLaunchKernelGGL (lt_tract_key_kernel, dim3 (grid_for (nt)), dim3 (256), 0, c->stream, tracts, nt, n, (const u64 *) d_keys, (const long long *) total,
                      (const Location *) d_loc, key[0], val[0], err);
  rc = kv_sort (c, key, val, nt, 8 * LT_KEY_PASSES);
  if (rc) return -rc;
  hipLaunchKernelGGL (lt_head_kernel, dim3 (grid_for (nt)), dim3 (256), 0, c->stream, (const u64 *) key[0], (const u32 *) val[0], nt, tracts, head, rows);
  rc = exclusive_scan (c, head, hex, nt, n_out);
  if (!rc) rc = exclusive_scan (c, rows, rowstart, nt, nullptr);
  if (rc) return -rc;
  hipLaunchKernelGGL (lt_perm_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, n, nt, (const u32 *) rowstart, (const u32 *) val[0], tracts,
                      (const u64 *) d_keys, d_perm, (u64 *) d_out_keys);
  if (d_out_counts)
    hipLaunchKernelGGL (lt_gather_counts_kernel, dim3 (grid_for (n * (long) n_samples)), dim3 (256), 0, c->stream, (const int *) d_counts, (const int *) d_perm, n, n_samples,
                        (int *) d_out_counts);
  hipLaunchKernelGGL (lt_merge_kernel, dim3 (grid_for (nt)), dim3 (256), 0, c->stream, nt, n, (const u32 *) head, (const u32 *) hex, (const u32 *) rowstart,
                      (const u32 *) val[0], tracts, (const long long *) total, (const Location *) d_loc, capacity, (UnionTract *) d_out_tracts,
                      (Location *) d_tract_loc, d_ref_length);
  st.end ();
  u32 h[2] = {0, 0};
  rc = read_back (c, fn, tot, h, 2);
  if (rc) return -rc;
  if (h[1] == 2) return -set_err (TJAMD_ERR_ARG, "%s: a location with flat >= 2^45", fn);
  if (h[1]) return -set_err (TJAMD_ERR_ARG, TILING_REFUSED, fn);
  if ((long) h[0] > capacity) return -set_err (TJAMD_ERR_CAPACITY, "%s: %u tracts, caller capacity %ld", fn, h[0], capacity);
  st.done ();
  return (long) h[0];
}
TJ_LAST_MS (tjamd_last_located_tracts_ms, T_LOCATED_TRACTS)

// ---- N8: per-sample tract variants against the reference ---------------------------------------------------------------
// The VCF step of the reference (update_vcf_file_from_context_histogram, find_ref_alt_ht_variants_from_strings,
// get_next_ht_location_from_same_contig, src/analyse_variable_tracts.c:147-233) on the permuted union of
// tjamd_located_tracts; the rule is in include/tatajuba_variants.h above tjamd_tract_variants.  The index entry at a tract's
// location holds the genome's flanks in the packing of the union rows, so the reference's comparison of two strings is word
// arithmetic (row_right_flank).  Segment mapping of union_tract_stats_kernel: S lanes per listed tract, a lane per sample (looping
// beyond 64); what they share -- tract_rows, located_tract -- is found by the segment's first lane and broadcast.
// Two passes of one kernel around an exclusive scan in sample-major order: flags, then records at their scanned places, so
// a record's place never depends on the order of atomics.  DESIGN.md section 3.5, N8.

struct Variant { long long flat; int tract, sample, contig, pos, row, base, ref_length, alt_length, n_flank, pad; u64 ref_flank, alt_flank; };
static_assert (sizeof (Variant) == 64 && sizeof (Variant) == sizeof (tjamd_variant), "variant layout");

// the entry at flat (ascending flat, one run per position), -1 if there is none
__device__ __forceinline__ long ref_entry_at (const RefEntry *__restrict__ entries, long n_ent, long long flat)
{
  long lo = 0, hi = n_ent;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (entries[mid].flat < flat) lo = mid + 1; else hi = mid;
  }
  return (lo < n_ent && entries[lo].flat == flat) ? lo : -1l;
}

// A located tract (N8, N13; run by a segment's first lane): the entry at tract t's location, -1 where it has no location or no
// entry sits there, and k_eff, the bases of its right flank that the next tract of the same contig leaves (k where none is near)
__device__ __forceinline__ long located_tract (const Location *__restrict__ tloc, long n_tracts, long t, const RefEntry *__restrict__ entries, long n_ent, int k, int &k_eff)
{
  const Location l = tloc[t];
  const long ent = l.flat >= 0 ? ref_entry_at (entries, n_ent, l.flat) : -1l;
  k_eff = ent < 0 ? 0 : k;
  if (ent >= 0 && t + 1 < n_tracts) {                   // stop at the next tract of the contig, whether a caller lists it or not
    const Location nx = tloc[t + 1];
    const long overlap = (long) l.pos + (long) entries[ent].length + (long) k - (long) nx.pos;
    if (nx.flat >= 0 && nx.contig == l.contig && overlap > 0) k_eff = (int) max (0l, (long) k - overlap);
  }
  return ent;
}

// The allele rule, which the VCF output rests on.  entry_right_flank: the forward right flank of an entry.  row_right_flank: that
// of a union row on the entry's strand, and n_flank: how many of its first k_eff bases hold every difference from fr, the outermost
// one and everything inside it (kmask: all ones at 32 bases, nothing at 0 -- no shift by 64)
__device__ __forceinline__ u64 entry_right_flank (const RefEntry &e, int k) { return e.neg_strand ? revcomp_k (e.ctx0, k) : e.ctx1; }
__device__ __forceinline__ u64 row_right_flank (const u64 *__restrict__ keys, long row, int neg, int k, int k_eff, u64 fr, int &n_flank)
{
  const u64 fa = neg ? revcomp_k (keys[3 * row], k) : keys[3 * row + 1];
  const u64 x = (fr ^ fa) & kmask (k_eff);
  n_flank = x ? (63 - __clzll ((long long) x)) / 2 + 1 : 0;
  return fa;
}

// a sample's modal row among rows [first, end) of the union: the highest count above 0, the first on a tie; -1 if it has none
// (the "sample's allele" of N8 and the max_length of N9)
__device__ __forceinline__ long modal_row (const int *__restrict__ counts, long first, long end, int ns, int s)
{
  int best = 0;
  long row = -1;
  for (long r = first; r < end; r++) {
    const int x = counts[r * ns + s];
    if (x > best) { best = x; row = r; }
  }
  return row;
}

// !WRITE: flag[s * n_list + i] = 1 where sample s has a call in list entry i (every word is written), and the checks:
// err |= 1 where the tracts do not tile the union, err |= 2 for a list id outside [0, n_tracts) (nothing is read outside the
// arrays either way).  WRITE: the records, at excl[s * n_list + i], those below capacity.
template <bool WRITE>
__global__ __launch_bounds__ (256)
void tract_variants_kernel (const u64 *__restrict__ keys, const int *__restrict__ counts, long n_union, int ns, int S, int k,
                            const UnionTract *__restrict__ tracts, long n_tracts, const Location *__restrict__ tloc,
                            const RefEntry *__restrict__ entries, long n_ent, const int *__restrict__ list, long n_list,
                            u32 *__restrict__ flag, const u32 *__restrict__ excl, Variant *__restrict__ out, long capacity, int *__restrict__ err)
{
  const long gthread = blockIdx.x * (long) blockDim.x + threadIdx.x, n_threads = (long) gridDim.x * blockDim.x;
  if (!WRITE) check_tiling (tracts, n_tracts, n_union, err);
  const int lane = threadIdx.x & (S - 1);
  const long segs_per_grid = n_threads / S;              // (its own spelling, not SEGMENT_MAP's: a 64-bit division, and this kernel's code as it was)
  for (long i = gthread / S; i < n_list; i += segs_per_grid) {   // (uniform across a segment)
    const long t = list ? (long) list[i] : i;
    long first = 0, end = 0, ent = -1;
    int k_eff = 0;
    if (lane == 0) {
      if (t < 0 || t >= n_tracts) { if (!WRITE) atomicOr (err, 2); }
      else tract_rows (tracts[t], n_union, first, end);   // (none of a broken tiling, flagged above: then no entry either)
      if (first < end) ent = located_tract (tloc, n_tracts, t, entries, n_ent, k, k_eff);
    }
    first = __shfl (first, 0, S); end = __shfl (end, 0, S); ent = __shfl (ent, 0, S); k_eff = __shfl (k_eff, 0, S);
    for (int s = lane; s < ns; s += S) {
      bool call = false;
      Variant v;
      if (ent >= 0) {
        const long row = modal_row (counts, first, end, ns, s);
        if (row >= 0) {
          const RefEntry e = entries[ent];
          const int La = meta_len (keys[3 * row + 2]), Lr = e.length;
          call = La >= 1 && La != Lr;
          if (WRITE && call) {
            const Location l = tloc[t];
            int nf;
            const u64 fr = entry_right_flank (e, k), fa = row_right_flank (keys, row, e.neg_strand, k, k_eff, fr, nf);
            v.flat = l.flat; v.tract = (int) t; v.sample = s; v.contig = l.contig; v.pos = l.pos + min (La, Lr);
            v.row = (int) row; v.base = e.neg_strand ? 3 - e.base : e.base; v.ref_length = Lr; v.alt_length = La;
            v.n_flank = nf; v.pad = 0; v.ref_flank = fr & kmask (nf); v.alt_flank = fa & kmask (nf);
          }
        }
      }
      const long at = (long) s * n_list + i;
      if (!WRITE) flag[at] = call ? 1u : 0u;
      else if (call && (long) excl[at] < capacity) out[excl[at]] = v;
    }
  }
}

// where each sample's records start: the scanned flags at the head of its stretch
__global__ void variant_offsets_kernel (const u32 *__restrict__ excl, long n_list, int ns, u32 *__restrict__ offs)
{
  for (long s = blockIdx.x * (long) blockDim.x + threadIdx.x; s < ns; s += (long) gridDim.x * blockDim.x) offs[s] = excl[s * n_list];
}

extern "C" long tjamd_tract_variants (tjamd_counter *c, const tjamd_reference *ref, const void *d_keys, const void *d_counts, long n_union,
                                      int n_samples, const tjamd_union_tract *d_tracts, long n_tracts, const tjamd_location *d_tract_loc,
                                      const int *d_list, long n_list, tjamd_variant *d_out, long capacity, long *h_offsets)
{
  static const char *fn = "tjamd_tract_variants";
  int rc = tiled_union_args (fn, d_keys, d_counts, n_union, n_samples, d_tracts, n_tracts, d_tract_loc);
  if (rc) return -rc;
  if (!d_list) n_list = n_tracts;                       // every tract
  if (n_list < 0) return -set_err (TJAMD_ERR_ARG, "%s: n_list %ld < 0", fn, n_list);
  if (capacity < 0 || (capacity > 0 && !d_out)) return -set_err (TJAMD_ERR_ARG, "%s: capacity %ld with %s record buffer", fn, capacity, d_out ? "a" : "a null");
  if (!h_offsets) return -set_err (TJAMD_ERR_ARG, "%s: null offsets", fn);
  if (!c || !ref) return -set_err (TJAMD_ERR_ARG, "%s: null counter or reference", fn);
  const long n_flags = n_list * (long) n_samples;
  if (n_flags >= (1l << 31)) return -set_err (TJAMD_ERR_CAPACITY, "%s: %ld listed tracts x %d samples", fn, n_list, n_samples);
  if (tjamd_device_count () <= 0) return -set_err (TJAMD_ERR_NO_DEVICE, "%s: TJAMD_ERR_NO_DEVICE: no HIP device visible (the variants are called on the device; no CPU fallback)", fn);
  if (const int bad = reference_of_counter (fn, ref, c)) return -bad;
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  Stage st (c, T_VARIANTS);
  if (n_flags == 0) {
    for (int s = 0; s <= n_samples; s++) h_offsets[s] = 0;
    return 0;
  }
  ScratchCut cut;
  u32 *flag, *excl, *offs;
  cut.take (flag, n_flags); cut.take (excl, n_flags); cut.take (offs, (size_t) n_samples + 2);
  rc = cut.commit (c);
  if (!rc) rc = ensure (c->scan_tmp, scan_tmp_words (n_flags) * 4 + 64, c->stream);
  if (rc) return -rc;
  u32 *total = offs + n_samples;                        // offs: the samples' starts, the number of records, the error flag
  int *err = (int *) (offs + n_samples + 1);
  if (hipMemsetAsync (total, 0, 8, c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: memset failed", fn);
  st.begin ();
  const int S = tract_segment (n_samples);
  auto launch = [&] (auto kernel) {
    hipLaunchKernelGGL (kernel, dim3 (tract_grid (n_list, S)), dim3 (256), 0, c->stream, (const u64 *) d_keys, (const int *) d_counts, n_union, n_samples, S, c->k,
                        (const UnionTract *) d_tracts, n_tracts, (const Location *) d_tract_loc, (const RefEntry *) ref->entries, ref->n_entries, d_list, n_list,
                        flag, (const u32 *) excl, (Variant *) d_out, capacity, err);
  };
  launch (tract_variants_kernel<false>);
  if (hipGetLastError () != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: launch failed", fn);
  rc = exclusive_scan (c, flag, excl, n_flags, total);
  if (rc) return -rc;
  hipLaunchKernelGGL (variant_offsets_kernel, dim3 (grid_for (n_samples)), dim3 (256), 0, c->stream, (const u32 *) excl, n_list, n_samples, offs);
  launch (tract_variants_kernel<true>);                 // (guarded by capacity: the count is only read for the check below)
  st.end ();
  std::vector<u32> h ((size_t) n_samples + 2, 0u);
  rc = read_back (c, fn, offs, h.data (), h.size ());
  if (rc) return -rc;
  const u32 h_err = h[(size_t) n_samples + 1];
  const long n_rec = (long) h[(size_t) n_samples];
  if (h_err & 1u) return -set_err (TJAMD_ERR_ARG, TILING_REFUSED, fn);
  if (h_err & 2u) return -set_err (TJAMD_ERR_ARG, "%s: a listed tract id is outside [0, %ld)", fn, n_tracts);
  if (n_rec > capacity) return -set_err (TJAMD_ERR_CAPACITY, "%s: %ld records, caller capacity %ld", fn, n_rec, capacity);
  for (int s = 0; s <= n_samples; s++) h_offsets[s] = (long) h[(size_t) s];
  st.done ();
  return n_rec;
}
TJ_LAST_MS (tjamd_last_tract_variants_ms, T_VARIANTS)

// ---- N9: the GFF3 feature a located tract lies in, and the longest modal length ------------------------------------------
// genomic_context_find_features (src/context_histogram.c:331-351) asks, per located histogram, for the features that hold
// the tract's first base, skips regions, keeps the last one and stops at the first CDS; the rule as built is in
// include/tatajuba_features.h.  Here the features become an elementary-interval table once (tjamd_annotation): the sorted
// start and end + 1 points of the features that are not regions, and per index the maximum of a priority that encodes the
// rule (a CDS above everything else, the earlier CDS above the later, otherwise the later feature above the earlier).  A
// tract is then one binary search, whatever the nesting depth and however long the features around it are.
// Thread mapping of the build, as in locate_kernel: a lane per feature finds its range of indices by two binary searches
// and paints a range of up to AN_LANE_PAINT indices by itself; a longer one (a gene over thousands of points) is handed
// to the whole wavefront, which paints it as consecutive words -- its length over 64, not one lane's serial walk.  The
// atomicMax decides a value, never a place, and a maximum does not depend on order: the table is the same from run to run.
// DESIGN.md section 3.5, N9.

struct Feature { int contig, start, end, cls, strand, line, type_off, id_off; };
static_assert (sizeof (Feature) == 32 && sizeof (Feature) == sizeof (tjamd_feature), "feature layout");
struct TractFeature { int feature, max_length; };
static_assert (sizeof (TractFeature) == 8 && sizeof (TractFeature) == sizeof (tjamd_tract_feature), "tract feature layout");

#define AN_LANE_PAINT   16
#define AN_MAX_FEATURES (1l << 30)      // the priorities of file indices below 2^30 stay apart in 31 bits

struct tjamd_annotation
{
  int device = 0;
  long n_features = 0, n_points = 0;
  u64 *points = nullptr;                // ascending, duplicates kept
  u32 *prio = nullptr;                  // per index e, for [points[e], points[e + 1]): the highest priority that covers it, 0 = nothing
};

__device__ __forceinline__ u64 feature_point (int contig, u32 at) { return ((u64) (u32) contig << 32) | (u64) at; }
__host__ __device__ __forceinline__ int priority_winner (u32 p) { return !p ? -1 : (p >> 31) ? (int) (0x7fffffffu - (p & 0x7fffffffu)) : (int) (p - 1u); }

__global__ void an_flag_kernel (const Feature *__restrict__ f, long n, u32 *__restrict__ flag)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) flag[i] = f[i].cls != TJAMD_FEATURE_REGION ? 1u : 0u;
}

// the two points of every feature that is not a region, at twice its rank among those
__global__ void an_points_kernel (const Feature *__restrict__ f, long n, const u32 *__restrict__ excl, u64 *__restrict__ key, u32 *__restrict__ val)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    const Feature x = f[i];
    if (x.cls == TJAMD_FEATURE_REGION) continue;
    const long j = 2l * excl[i];
    key[j] = feature_point (x.contig, (u32) x.start); key[j + 1] = feature_point (x.contig, (u32) x.end + 1u);
    val[j] = val[j + 1] = (u32) i;
  }
}

// first index of points[0, n) whose point is not below q (behind = false) / is above q (behind = true)
__device__ __forceinline__ long point_bound (const u64 *__restrict__ points, long n, u64 q, bool behind)
{
  long lo = 0, hi = n;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    const u64 p = points[mid];
    if (behind ? p <= q : p < q) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__ (256)
void an_paint_kernel (const Feature *__restrict__ f, long n, const u64 *__restrict__ points, long np, u32 *__restrict__ prio)
{
  const int lane = threadIdx.x & 63;
  const long stride = (long) gridDim.x * blockDim.x;
  for (long i0 = blockIdx.x * (long) blockDim.x + (threadIdx.x & ~63); i0 < n; i0 += stride) {     // (uniform across a wavefront)
    const long i = i0 + lane;
    long lo = 0, hi = 0;
    u32 p = 0;
    if (i < n) {
      const Feature x = f[i];
      if (x.cls != TJAMD_FEATURE_REGION) {
        lo = point_bound (points, np, feature_point (x.contig, (u32) x.start), false);
        hi = point_bound (points, np, feature_point (x.contig, (u32) x.end + 1u), false);
        p = x.cls == TJAMD_FEATURE_CDS ? (1u << 31) | (0x7fffffffu - (u32) i) : (u32) i + 1u;
      }
    }
    const bool mine = hi - lo <= AN_LANE_PAINT;
    if (mine) for (long e = lo; e < hi; e++) atomicMax (&prio[e], p);
    u64 big = __ballot (!mine);
    while (big) {                                       // the wavefront paints its long ranges together, one after the other
      const int src = __ffsll ((long long) big) - 1;
      big &= big - 1;
      const long blo = __shfl (lo, src), bhi = __shfl (hi, src);
      const u32 bp = __shfl (p, src);
      for (long e = blo + lane; e < bhi; e += 64) atomicMax (&prio[e], bp);
    }
  }
}

extern "C" void tjamd_annotation_destroy (tjamd_annotation *a)
{
  if (!a) return;
  (void) hipSetDevice (a->device);
  if (a->points) (void) hipFree (a->points);
  if (a->prio) (void) hipFree (a->prio);
  delete a;
}

extern "C" tjamd_annotation *tjamd_annotation_create (tjamd_counter *c, const tjamd_reference *ref, const tjamd_feature *h_features, long n_features)
{
  static const char *fn = "tjamd_annotation_create";
  auto refused = [&] () -> int {                        // the checks that read no handle, the devices last
    if (!c || !ref) return set_err (TJAMD_ERR_ARG, "%s: null counter or reference", fn);
    if (n_features < 0 || (n_features > 0 && !h_features)) return set_err (TJAMD_ERR_ARG, "%s: %ld features with %s buffer", fn, n_features, h_features ? "a" : "a null");
    if (n_features > AN_MAX_FEATURES) return set_err (TJAMD_ERR_ARG, "%s: %ld features, more than 2^30", fn, n_features);
    if (tjamd_device_count () <= 0) return set_err (TJAMD_ERR_NO_DEVICE, "%s: TJAMD_ERR_NO_DEVICE: no HIP device visible (the table is built on the device; no CPU fallback)", fn);
    return on_counter_device (fn, "reference", ref->device, c);
  };
  const int bad = refused ();
  Stage st (c, T_ANNOTATION);                           // (a refused call leaves no timing behind)
  if (bad) return NULL;
  const long n = n_features;
  long nr = 0;                                          // features that are not regions
  for (long i = 0; i < n; i++) {
    const tjamd_feature &x = h_features[i];
    if (feature_refused (fn, i, x, ref->n_contigs)) return NULL;
    if (x.cls < 0 || x.cls > 2) { set_err (TJAMD_ERR_ARG, "%s: feature %ld: cls %d outside 0..2", fn, i, x.cls); return NULL; }
    nr += x.cls != TJAMD_FEATURE_REGION;
  }
  HIPCHK_NULL (hipSetDevice (c->device));
  std::unique_ptr<tjamd_annotation, void (*) (tjamd_annotation *)> a (new tjamd_annotation (), tjamd_annotation_destroy);
  a->device = c->device; a->n_features = n; a->n_points = 2 * nr;
  const long np = a->n_points;
  ScratchCut cut;
  Feature *feat; u32 *flag, *excl, *val[2]; u64 *key[2];
  cut.take (feat, n + 1); cut.take (flag, n + 1); cut.take (excl, n + 1);
  cut.take (key[0], np + 1); cut.take (key[1], np + 1); cut.take (val[0], np + 1); cut.take (val[1], np + 1);
  if (cut.commit (c) || reserve_sort (c, np, n)) return NULL;
  if (np && (hipMalloc (&a->points, (size_t) np * 8) != hipSuccess || hipMalloc (&a->prio, (size_t) np * 4) != hipSuccess)) { set_err (TJAMD_ERR_HIP, "%s: hipMalloc failed for %ld points", fn, np); return NULL; }
  if (n && hipMemcpyAsync (feat, h_features, (size_t) n * sizeof (Feature), hipMemcpyHostToDevice, c->stream) != hipSuccess) { set_err (TJAMD_ERR_HIP, "%s: copy to device failed", fn); return NULL; }
  if (np && hipMemsetAsync (a->prio, 0, (size_t) np * 4, c->stream) != hipSuccess) { set_err (TJAMD_ERR_HIP, "%s: memset failed", fn); return NULL; }
  st.begin ();
  hipLaunchKernelGGL (an_flag_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const Feature *) feat, n, flag);
  if (np) {
    int rc = exclusive_scan (c, flag, excl, n, nullptr);
    hipLaunchKernelGGL (an_points_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const Feature *) feat, n, (const u32 *) excl, key[0], val[0]);
    int bits = 32;                                      // of a point: the position, and what the contig numbers need
    while (bits < 64 && ((u64) (ref->n_contigs - 1) >> (bits - 32))) bits++;
    if (!rc) rc = kv_sort (c, key, val, np, bits);
    if (rc) return NULL;
    hipLaunchKernelGGL (an_paint_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const Feature *) feat, n, (const u64 *) key[0], np, a->prio);
  }
  st.end ();
  if (np && hipMemcpyAsync (a->points, key[0], (size_t) np * 8, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) { set_err (TJAMD_ERR_HIP, "%s: copy of the points failed", fn); return NULL; }
  if (read_back (c, fn, nullptr, nullptr, 0)) return NULL;
  st.done ();
  return a.release ();
}

extern "C" long tjamd_annotation_features (const tjamd_annotation *a) { return a ? a->n_features : -1; }

extern "C" long tjamd_annotation_download (const tjamd_annotation *a, uint64_t *h_points, int *h_winner, long capacity)
{
  static const char *fn = "tjamd_annotation_download";
  if (!a) return -set_err (TJAMD_ERR_ARG, "%s: null annotation", fn);
  const long np = a->n_points;
  if (np == 0 || capacity < np) return np;
  if (!h_points || !h_winner) return -set_err (TJAMD_ERR_ARG, "%s: null buffer", fn);
  std::vector<u32> prio ((size_t) np);
  if (hipSetDevice (a->device) != hipSuccess || hipMemcpy (h_points, a->points, (size_t) np * 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy (prio.data (), a->prio, (size_t) np * 4, hipMemcpyDeviceToHost) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: copy failed", fn);
  for (long e = 0; e < np; e++) h_winner[e] = priority_winner (prio[(size_t) e]);
  return np;
}
TJ_LAST_MS (tjamd_last_annotation_ms, T_ANNOTATION)

// One record per tract.  Segment mapping of union_tract_stats_kernel and tract_variants_kernel: S lanes per tract; the
// segment's first lane looks the location up in the table (one binary search) and reads the tract's rows; with a union, a
// lane per sample (looping beyond 64) takes the length of the sample's modal row and the segment reduces the maximum with
// shuffles.  Without a union (keys == NULL, S = 1) a thread per tract does the lookup alone.  err |= 1: the tracts do not
// tile the union (tiling_check_kernel, a launch of its own in front: the lookup returns while the flag is up, so a refused call
// writes nothing; tract_rows reads nothing outside the arrays either way).
__global__ void tiling_check_kernel (const UnionTract *__restrict__ tracts, long n_tracts, long n_union, int *__restrict__ err)
{
  check_tiling (tracts, n_tracts, n_union, err);
}

__global__ __launch_bounds__ (256)
void tract_features_kernel (const u64 *__restrict__ keys, const int *__restrict__ counts, long n_union, int ns, int S,
                            const UnionTract *__restrict__ tracts, long n_tracts, const Location *__restrict__ tloc,
                            const u64 *__restrict__ points, const u32 *__restrict__ prio, long np, TractFeature *__restrict__ out, int *__restrict__ err)
{
  const long gthread = blockIdx.x * (long) blockDim.x + threadIdx.x, n_threads = (long) gridDim.x * blockDim.x;
  if (*(volatile int *) err != 0) return;                // (the check is complete: every thread reads the same word)
  const int lane = threadIdx.x & (S - 1);
  const long segs_per_grid = n_threads / S;              // (its own spelling, not SEGMENT_MAP's: a 64-bit division, and this kernel's code as it was)
  for (long t = gthread / S; t < n_tracts; t += segs_per_grid) {   // (uniform across a segment)
    int feature = -1, longest = 0;
    long first = 0, end = 0;
    if (lane == 0) {
      const Location l = tloc[t];
      if (l.flat >= 0 && l.contig >= 0 && l.pos >= 0) {
        const long e = point_bound (points, np, feature_point (l.contig, (u32) l.pos + 1u), true) - 1;
        if (e >= 0) feature = priority_winner (prio[e]);
      }
      if (keys) tract_rows (tracts[t], n_union, first, end);   // (none of a broken tiling: flagged above)
    }
    if (keys) {
      first = __shfl (first, 0, S); end = __shfl (end, 0, S);
      int best = INT_MIN;                               // (a length field may read negative: no sample is not length 0)
      for (int s = lane; s < ns; s += S) {
        const long row = modal_row (counts, first, end, ns, s);
        if (row >= 0) best = max (best, meta_len (keys[3 * row + 2]));
      }
      for (int o = 1; o < S; o <<= 1) best = max (best, __shfl_xor (best, o, S));
      longest = best == INT_MIN ? 0 : best;
    }
    if (lane == 0) out[t] = TractFeature {feature, longest};
  }
}

extern "C" long tjamd_tract_features (tjamd_counter *c, const tjamd_annotation *a, const void *d_keys, const void *d_counts, long n_union,
                                      int n_samples, const tjamd_union_tract *d_tracts, long n_tracts, const tjamd_location *d_tract_loc,
                                      tjamd_tract_feature *d_out)
{
  static const char *fn = "tjamd_tract_features";
  const bool have_union = d_keys && d_counts;
  auto refused = [&] () -> int {                        // the checks that read no handle, the counter's device last
    if (have_union) {
      int rc = union_args (fn, d_keys, d_counts, n_union, n_samples);   // (the locations are checked with the output, below: not tiled_union_args)
      if (!rc) rc = tract_count_arg (fn, n_tracts, n_union);
      if (rc) return rc;
      if (n_tracts > 0 && !d_tracts) return set_err (TJAMD_ERR_ARG, "%s: null tract buffer", fn);
    }
    if (n_tracts < 0) return set_err (TJAMD_ERR_ARG, "%s: n_tracts %ld < 0", fn, n_tracts);
    if (n_tracts >= (1l << 31)) return set_err (TJAMD_ERR_CAPACITY, "%s: %ld tracts", fn, n_tracts);
    if (n_tracts > 0 && (!d_tract_loc || !d_out)) return set_err (TJAMD_ERR_ARG, "%s: null tract location or output buffer", fn);
    if (!c || !a) return set_err (TJAMD_ERR_ARG, "%s: null counter or annotation", fn);
    if (tjamd_device_count () <= 0) return set_err (TJAMD_ERR_NO_DEVICE, "%s: TJAMD_ERR_NO_DEVICE: no HIP device visible (the tracts are looked up on the device; no CPU fallback)", fn);
    return on_counter_device (fn, "annotation", a->device, c);
  };
  int rc = refused ();
  Stage st (c, T_TRACT_FEATURES);                       // (a refused call leaves no timing behind)
  if (rc) return -rc;
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  if (n_tracts == 0) return 0;
  int *err;
  rc = flags_alone (c, fn, err);
  if (rc) return -rc;
  st.begin ();
  const int S = have_union ? tract_segment (n_samples) : 1;
  if (have_union) hipLaunchKernelGGL (tiling_check_kernel, dim3 (grid_for (n_tracts)), dim3 (256), 0, c->stream, (const UnionTract *) d_tracts, n_tracts, n_union, err);
  hipLaunchKernelGGL (tract_features_kernel, dim3 (tract_grid (n_tracts, S)), dim3 (256), 0, c->stream, have_union ? (const u64 *) d_keys : (const u64 *) nullptr,
                      (const int *) d_counts, n_union, n_samples, S, (const UnionTract *) d_tracts, n_tracts, (const Location *) d_tract_loc,
                      (const u64 *) a->points, (const u32 *) a->prio, a->n_points, (TractFeature *) d_out, err);
  st.end ();
  int h_err = 0;
  rc = read_back (c, fn, err, &h_err, 1);
  if (rc) return -rc;
  if (h_err) return -set_err (TJAMD_ERR_ARG, TILING_REFUSED, fn);
  st.done ();
  return n_tracts;
}
TJ_LAST_MS (tjamd_last_tract_features_ms, T_TRACT_FEATURES)

// ---- N11: the coding effect of a variant record ---------------------------------------------------------------------------
// The rule is in include/tatajuba_effects.h.  The table (tjamd_coding) keeps the genome as one code per byte, the contig
// starts and one row per feature: the clipped span and, for a coding feature, where its protein ends.  The lookup
// (variant_effects_kernel) classifies a record by translating the reference and the alternative sequence from the edit's codon
// on.  Thread mapping of both kernels, as in locate_kernel and an_paint_kernel: the serial part of one item (a CDS's scan for
// its stop, a record's walk to the alternative's stop) belongs to the whole wavefront, 64 consecutive codons per step, so
// its time is the item's length over 64 and not one lane's walk while 63 wait.  DESIGN.md section 3.5, N11.

struct Cds { int aa_len, has_stop, n_codons, phase; };
static_assert (sizeof (Cds) == 16 && sizeof (Cds) == sizeof (tjamd_cds), "cds layout");
struct Effect { int feature, cls, cds_pos, first_diff, ref_aa_len, alt_aa_len, flags, pad; u64 ref_aa, alt_aa; };
static_assert (sizeof (Effect) == 48 && sizeof (Effect) == sizeof (tjamd_effect), "effect layout");
// a feature's row: its tjamd_cds, then the span as the lookup needs it (start is the 0-based S, len the clipped length)
struct CodRow { Cds cds; int start, len, contig, strand; };
static_assert (sizeof (CodRow) == 32, "coding row layout");

#define CD_MAX_FEATURES (1l << 30)
#define CD_STOPS 0x0105000000000000ull  // bit i: codon index i is a stop (TAA = 48, TAG = 50, TGA = 56)

// the code of a base: A C G T/U in either case are 0 to 3, every other byte is 4
__host__ __device__ __forceinline__ u32 base_code5 (u32 b)
{
  const u32 l = b | 0x20u;
  return l == 'a' ? 0u : l == 'c' ? 1u : l == 'g' ? 2u : (l == 't' || l == 'u') ? 3u : 4u;
}
__host__ __device__ __forceinline__ u32 code_complement (u32 c) { return c < 4u ? 3u - c : 4u; }

// The standard genetic code by codon index b0 << 4 | b1 << 2 | b2 (A, C, G, T = 0 .. 3), written out from its definition:
// third-base families (ACx T, CCx P, CGx R, CTx L, GCx A, GGx G, GTx V, TCx S), the purine / pyrimidine pairs (AAr K, AAy N, AGr
// R, AGy S, CAr Q, CAy H, GAr E, GAy D, TAy Y, TGy C, TTr L, TTy F), ATA ATC ATT I, ATG M, TGG W, and the stops TAA TAG TGA.
__host__ __device__ __forceinline__ char aa_table_byte (u32 i)
{
  return "KNKNTTTTRSRSIIMI" "QHQHPPPPRRRRLLLL" "EDEDAAAAGGGGVVVV" "*Y*YSSSS*CWCLFLF"[i & 63u];
}
// the amino acid of three codes; tab holds the 64 bytes of aa_table_byte (on the device a copy in LDS: the lanes of a
// wavefront index it apart).  The one routine of tjamd_translate and of the kernels.
__host__ __device__ __forceinline__ u32 amino_acid (const char *tab, u32 b0, u32 b1, u32 b2)
{
  return (b0 | b1 | b2) > 3u ? (u32) 'X' : (u32) (unsigned char) tab[(b0 << 4) | (b1 << 2) | b2];
}
__host__ __device__ __forceinline__ bool codon_is_stop (u32 b0, u32 b1, u32 b2)
{
  return (b0 | b1 | b2) <= 3u && ((CD_STOPS >> ((b0 << 4) | (b1 << 2) | b2)) & 1ull);
}

extern "C" long tjamd_translate (const char *dna, long n, int reverse, char *out, long capacity)
{
  static const char *fn = "tjamd_translate";
  if (n < 0) return -set_err (TJAMD_ERR_ARG, "%s: n %ld < 0", fn, n);
  if (n > 0 && !dna) return -set_err (TJAMD_ERR_ARG, "%s: null dna", fn);
  const long na = n / 3;
  if (capacity < na) return na;
  if (na > 0 && !out) return -set_err (TJAMD_ERR_ARG, "%s: null output buffer", fn);
  char tab[64];
  for (u32 i = 0; i < 64u; i++) tab[i] = aa_table_byte (i);
  auto code = [&] (long j) -> u32 { return reverse ? code_complement (base_code5 ((unsigned char) dna[n - 1 - j])) : base_code5 ((unsigned char) dna[j]); };
  for (long i = 0; i < na; i++) out[i] = (char) amino_acid (tab, code (3 * i), code (3 * i + 1), code (3 * i + 2));
  return na;
}

struct tjamd_coding
{
  int device = 0;
  long n_features = 0, n_contigs = 0, n_bytes = 0;
  uint8_t *codes = nullptr;             // one code per byte of the stream (a delimiter is a 4 like any other byte that is no base)
  u32 *cstart = nullptr;                // [n_contigs + 1]: contig c begins at cstart[c] and is cstart[c + 1] - 1 - cstart[c] long
  CodRow *rows = nullptr;               // [n_features]
};

// one code per byte; the delimiters flagged for the scan that numbers the contigs
__global__ void cd_code_kernel (const uint8_t *__restrict__ seq, long n, uint8_t *__restrict__ codes, u32 *__restrict__ nlflag)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    const u32 b = seq[i];
    codes[i] = (uint8_t) base_code5 (b);
    nlflag[i] = b == '\n' ? 1u : 0u;
  }
}

// cstart[0] = 0; behind the c-th delimiter begins contig c; a last contig without a delimiter ends as if one stood at n
__global__ void cd_cstart_kernel (const uint8_t *__restrict__ seq, long n, const u32 *__restrict__ nlflag, const u32 *__restrict__ nlex, u32 *__restrict__ cstart)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    if (i == 0) cstart[0] = 0u;
    if (nlflag[i]) cstart[nlex[i] + 1u] = (u32) i + 1u;
    else if (i == n - 1) cstart[nlex[i] + 1u] = (u32) n + 1u;
  }
}

// CDS-oriented base j of a span of len codes that begins at g: the span on strand 0, its reverse complement on strand 1
__device__ __forceinline__ u32 span_code (const uint8_t *__restrict__ g, long len, int strand, long j)
{
  return strand ? code_complement (g[len - 1 - j]) : (u32) g[j];
}

// One wavefront per feature.  A coding feature: 64 codons per step, lane l on codon 64 * step + l (192 consecutive bytes a
// step), a ballot of "is a stop" whose lowest bit is the first stop; the wavefront leaves at the first step that has one.
__global__ __launch_bounds__ (256)
void cds_scan_kernel (const uint8_t *__restrict__ codes, const u32 *__restrict__ cstart, const Feature *__restrict__ f, const signed char *__restrict__ phase,
                      long n, CodRow *__restrict__ rows)
{
  const int lane = threadIdx.x & 63;
  const long n_waves = (long) gridDim.x * (blockDim.x >> 6);
  for (long i = blockIdx.x * (long) (blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += n_waves) {     // (uniform across a wavefront)
    const Feature x = f[i];
    if (x.cls != TJAMD_FEATURE_CDS || (x.strand != 0 && x.strand != 1)) {
      if (lane == 0) rows[i] = CodRow {Cds {-1, -1, -1, -1}, x.start - 1, 0, x.contig, x.strand};
      continue;
    }
    const long c0 = cstart[x.contig], clen = (long) cstart[x.contig + 1] - 1 - c0;
    const long S = (long) x.start - 1, E = min ((long) x.end, clen) - 1, len = max (E - S + 1, 0l);
    int ph = phase ? (int) phase[i] : 0;
    if (ph != 1 && ph != 2) ph = 0;
    const long nc = max (len - ph, 0l) / 3;
    const uint8_t *g = codes + c0 + S;                  // (read only inside [0, len))
    long first_stop = -1;
    for (long at = 0; at < nc; at += 64) {
      const long cdn = at + lane;
      bool stop = false;
      if (cdn < nc) {
        const long j = 3 * cdn + ph;
        stop = codon_is_stop (span_code (g, len, x.strand, j), span_code (g, len, x.strand, j + 1), span_code (g, len, x.strand, j + 2));
      }
      const u64 m = __ballot (stop);
      if (m) { first_stop = at + __ffsll ((long long) m) - 1; break; }
    }
    if (lane == 0) rows[i] = CodRow {Cds {(int) (first_stop >= 0 ? first_stop : nc), first_stop >= 0 ? 1 : 0, (int) nc, ph}, (int) S, (int) len, x.contig, x.strand};
  }
}

extern "C" void tjamd_coding_destroy (tjamd_coding *cod)
{
  if (!cod) return;
  (void) hipSetDevice (cod->device);
  if (cod->codes) (void) hipFree (cod->codes);
  if (cod->cstart) (void) hipFree (cod->cstart);
  if (cod->rows) (void) hipFree (cod->rows);
  delete cod;
}

extern "C" tjamd_coding *tjamd_coding_create (tjamd_counter *c, const void *h_stream, size_t n_bytes,
                                              const tjamd_feature *h_features, long n_features, const signed char *h_phase)
{
  static const char *fn = "tjamd_coding_create";
  long n_contigs = 0;
  auto refused = [&] () -> int {                        // the checks that read no handle: the caller's host buffers, then the device
    if (!c) return set_err (TJAMD_ERR_ARG, "%s: null counter", fn);
    if (const int rc = stream_refused (fn, h_stream, n_bytes)) return rc;
    if (n_features < 0 || (n_features > 0 && !h_features)) return set_err (TJAMD_ERR_ARG, "%s: %ld features with %s buffer", fn, n_features, h_features ? "a" : "a null");
    if (n_features > CD_MAX_FEATURES) return set_err (TJAMD_ERR_ARG, "%s: %ld features, more than 2^30", fn, n_features);
    const char *s = (const char *) h_stream;
    for (size_t at = 0; at < n_bytes; n_contigs++) {
      const char *nl = (const char *) memchr (s + at, '\n', n_bytes - at);
      at = nl ? (size_t) (nl - s) + 1 : n_bytes;
    }
    for (long i = 0; i < n_features; i++) if (const int rc = feature_refused (fn, i, h_features[i], n_contigs)) return rc;
    if (tjamd_device_count () <= 0) return set_err (TJAMD_ERR_NO_DEVICE, "%s: TJAMD_ERR_NO_DEVICE: no HIP device visible (the table is built on the device; no CPU fallback)", fn);
    return TJAMD_OK;
  };
  const int bad = refused ();
  Stage st (c, T_CODING);                               // (a refused call leaves no timing behind)
  if (bad) return NULL;
  HIPCHK_NULL (hipSetDevice (c->device));
  std::unique_ptr<tjamd_coding, void (*) (tjamd_coding *)> cod (new tjamd_coding (), tjamd_coding_destroy);
  cod->device = c->device; cod->n_features = n_features; cod->n_contigs = n_contigs; cod->n_bytes = (long) n_bytes;
  const long n = (long) n_bytes, nf = n_features;
  ScratchCut cut;
  u32 *nlflag, *nlex; Feature *feat; signed char *phase;
  cut.take (nlflag, n + 1); cut.take (nlex, n + 1); cut.take (feat, nf + 1); cut.take (phase, nf + 1);
  if (cut.commit (c) || upload_stream (c, fn, h_stream, n_bytes) || ensure (c->scan_tmp, scan_tmp_words (n) * 4 + 64, c->stream)) return NULL;
  if (hipMalloc (&cod->codes, (size_t) std::max<long> (n, 1)) != hipSuccess || hipMalloc (&cod->cstart, (size_t) (n_contigs + 2) * 4) != hipSuccess ||
      hipMalloc (&cod->rows, (size_t) std::max<long> (nf, 1) * sizeof (CodRow)) != hipSuccess) { set_err (TJAMD_ERR_HIP, "%s: hipMalloc failed for %ld bytes of genome and %ld features", fn, n, nf); return NULL; }
  if ((nf && hipMemcpyAsync (feat, h_features, (size_t) nf * sizeof (Feature), hipMemcpyHostToDevice, c->stream) != hipSuccess) ||
      (nf && h_phase && hipMemcpyAsync (phase, h_phase, (size_t) nf, hipMemcpyHostToDevice, c->stream) != hipSuccess)) { set_err (TJAMD_ERR_HIP, "%s: copy to device failed", fn); return NULL; }
  st.begin ();
  if (n) {
    const uint8_t *seq = (const uint8_t *) c->stage.p;
    hipLaunchKernelGGL (cd_code_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, seq, n, cod->codes, nlflag);
    if (exclusive_scan (c, nlflag, nlex, n, nullptr)) return NULL;
    hipLaunchKernelGGL (cd_cstart_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, seq, n, (const u32 *) nlflag, (const u32 *) nlex, cod->cstart);
  }
  if (nf)                                               // (features need contigs, contigs need bytes: n > 0 here)
    hipLaunchKernelGGL (cds_scan_kernel, dim3 ((unsigned) std::min<long> ((nf + 3) / 4, 65536)), dim3 (256), 0, c->stream, (const uint8_t *) cod->codes,
                        (const u32 *) cod->cstart, (const Feature *) feat, h_phase ? (const signed char *) phase : (const signed char *) nullptr, nf, cod->rows);
  st.end ();
  if (read_back (c, fn, nullptr, nullptr, 0)) return NULL;
  st.done ();
  return cod.release ();
}

extern "C" long tjamd_coding_features (const tjamd_coding *cod) { return cod ? cod->n_features : -1; }

extern "C" long tjamd_coding_download (const tjamd_coding *cod, tjamd_cds *out, long capacity)
{
  static const char *fn = "tjamd_coding_download";
  if (!cod) return -set_err (TJAMD_ERR_ARG, "%s: null coding table", fn);
  const long nf = cod->n_features;
  if (nf == 0 || capacity < nf) return nf;
  if (!out) return -set_err (TJAMD_ERR_ARG, "%s: null buffer", fn);
  if (hipSetDevice (cod->device) != hipSuccess ||
      hipMemcpy2D (out, sizeof (Cds), cod->rows, sizeof (CodRow), sizeof (Cds), (size_t) nf, hipMemcpyDeviceToHost) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: copy failed", fn);
  return nf;
}
TJ_LAST_MS (tjamd_last_coding_ms, T_CODING)

// what the wavefront needs of an owner's record: the span, where the edit sits in it and what ALT is made of
struct Walk
{
  const uint8_t *g;                     // the span's first code (forward)
  long len, alt_len;                    // of the span, of the alternative span
  long e, n_ref, n_alt, n_run;          // the edit's offset in the span (p - S), |REF|, |ALT|, ALT's run of the base
  u32 base; u64 flank;                  // the run base, ALT's flank bases
  int strand, phase;
};

// CDS-oriented base j of the alternative span: a genome code, the run base or two bits of alt_flank, chosen by its index
__device__ __forceinline__ u32 alt_code (const Walk &w, long j)
{
  const long x = w.strand ? w.alt_len - 1 - j : j;      // forward index in the alternative span
  u32 cd;
  if (x < w.e) cd = w.g[x];
  else if (x < w.e + w.n_alt) { const long t = x - w.e; cd = t < w.n_run ? w.base : (u32) (w.flank >> (2 * (t - w.n_run))) & 3u; }
  else cd = w.g[x - w.n_alt + w.n_ref];
  return w.strand ? code_complement (cd) : cd;
}
__device__ __forceinline__ u32 ref_symbol (const Walk &w, const char *tab, long cdn)
{
  const long j = 3 * cdn + w.phase;
  return amino_acid (tab, span_code (w.g, w.len, w.strand, j), span_code (w.g, w.len, w.strand, j + 1), span_code (w.g, w.len, w.strand, j + 2));
}
__device__ __forceinline__ u32 alt_symbol (const Walk &w, const char *tab, long cdn)
{
  const long j = 3 * cdn + w.phase;
  return amino_acid (tab, alt_code (w, j), alt_code (w, j + 1), alt_code (w, j + 2));
}

// err bits: 1 contig, 2 pos or q, 4 n_flank, 8 a length, 16 tract, 32 feature index (tjamd_variant_effects names them)
// effect_record_bad: the bits of one record, with the record's feature, the start of its contig and the contig's length
__device__ __forceinline__ int effect_record_bad (const Variant &v, const u32 *__restrict__ cstart, long n_contigs, const TractFeature *__restrict__ tf, long n_tracts,
                                                  long n_features, int &f, long &c0, long &clen)
{
  int bad = 0;
  f = -1; c0 = 0; clen = 0;
  if (v.contig < 0 || (long) v.contig >= n_contigs) bad |= 1;
  else { c0 = cstart[v.contig]; clen = (long) cstart[v.contig + 1] - 1 - c0; }
  if (v.n_flank < 0 || v.n_flank > 32) bad |= 4;
  if (v.ref_length < 1 || v.alt_length < 1) bad |= 8;
  const long q = (long) v.pos - 1 + max ((long) v.ref_length - (long) v.alt_length, 0l) + (long) v.n_flank;
  if (!bad && (v.pos < 1 || q >= clen)) bad |= 2;
  if (tf) {
    if (v.tract < 0 || (long) v.tract >= n_tracts) bad |= 16;
    else { f = tf[v.tract].feature; if (f < -1 || (long) f >= n_features) { bad |= 32; f = -1; } }
  }
  return bad;
}

// every record's check, a launch of its own in front of the walk: variant_effects_kernel returns while the flag is up, so a
// refused call writes nothing
__global__ void variant_effects_check_kernel (const u32 *__restrict__ cstart, long n_contigs, long n_features, const Variant *__restrict__ var, long n,
                                              const TractFeature *__restrict__ tf, long n_tracts, int *__restrict__ err)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    int f; long c0, clen;
    const int bad = effect_record_bad (var[i], cstart, n_contigs, tf, n_tracts, n_features, f, c0, clen);
    if (bad) atomicOr (err, bad);
  }
}

__global__ __launch_bounds__ (256)
void variant_effects_kernel (const uint8_t *__restrict__ codes, const u32 *__restrict__ cstart, long n_contigs, const CodRow *__restrict__ rows, long n_features,
                             const Variant *__restrict__ var, long n, const TractFeature *__restrict__ tf, long n_tracts, Effect *__restrict__ out, int *__restrict__ err)
{
  __shared__ char tab[64];                              // the lanes index the amino acids apart: LDS, not a constant array
  if (*(volatile int *) err != 0) return;                // (the check is complete: every thread reads the same word)
  if (threadIdx.x < 64) tab[threadIdx.x] = aa_table_byte (threadIdx.x);
  __syncthreads ();
  const int lane = threadIdx.x & 63;
  const long stride = (long) gridDim.x * blockDim.x;
  for (long i0 = blockIdx.x * (long) blockDim.x + (threadIdx.x & ~63); i0 < n; i0 += stride) {     // (uniform across a wavefront)
    const long i = i0 + lane;
    bool walk = false;
    Walk w = {codes, 0, 0, 0, 0, 0, 0, 0u, 0ull, 0, 0};
    Effect r = {-1, TJAMD_EFFECT_NONE, 0, -1, 0, 0, 0, 0, 0ull, 0ull};
    long c_first = 0, p_ref = 0;                        // the walk's first codon; the symbols of P_ref
    int delta = 0;
    if (i < n) {
      const Variant v = var[i];
      int f;
      long clen, c0;
      const int bad = effect_record_bad (v, cstart, n_contigs, tf, n_tracts, n_features, f, c0, clen);
      const long Lr = v.ref_length, La = v.alt_length, nfl = v.n_flank;
      const long n_ref = max (Lr - La, 0l) + 1 + nfl, n_alt = max (La - Lr, 0l) + 1 + nfl;
      const long p = (long) v.pos - 1, q = p + n_ref - 1;
      if (!bad) {                                       // (a bad record has raised the flag in the check: this launch has returned)
        r.feature = f;
        CodRow row = {Cds {-1, -1, -1, -1}, 0, 0, 0, 0};
        if (f >= 0) row = rows[f];
        if (row.cds.aa_len >= 0) {
          const long S = row.start, E = S + row.len - 1;
          r.ref_aa_len = row.cds.aa_len; r.flags = row.cds.has_stop ? TJAMD_EFFECT_REF_STOP : 0;
          if (row.contig != v.contig || p < S || q > E) r.cls = TJAMD_EFFECT_BOUNDARY;
          else {
            walk = true;
            w.g = codes + c0 + S; w.len = row.len; w.alt_len = (long) row.len + n_alt - n_ref;
            w.e = p - S; w.n_ref = n_ref; w.n_alt = n_alt; w.n_run = max (La - Lr, 0l) + 1;
            w.base = (u32) v.base & 3u; w.flank = v.alt_flank; w.strand = row.strand; w.phase = row.cds.phase;
            r.cds_pos = (int) (row.strand ? E - q : p + 1 - S);
            const long same = row.strand ? E - q : p - S;                   // CDS-oriented bases in front of the edit: equal in both
            c_first = max (same - (long) row.cds.phase, 0l) / 3;
            p_ref = (long) row.cds.aa_len + row.cds.has_stop;
            delta = (int) ((La - Lr) % 3);
          }
        }
        if (!walk) out[i] = r;
      }
    }
    u64 owners = __ballot (walk);
    while (owners) {                                    // the wavefront walks its records together, one after the other
      const int src = __ffsll ((long long) owners) - 1;
      owners &= owners - 1;
      Walk o;
      o.g = (const uint8_t *) __shfl ((unsigned long long) w.g, src);
      o.len = __shfl (w.len, src); o.alt_len = __shfl (w.alt_len, src); o.e = __shfl (w.e, src); o.n_ref = __shfl (w.n_ref, src);
      o.n_alt = __shfl (w.n_alt, src); o.n_run = __shfl (w.n_run, src); o.base = __shfl (w.base, src); o.flank = __shfl (w.flank, src);
      o.strand = __shfl (w.strand, src); o.phase = __shfl (w.phase, src);
      const long first = __shfl (c_first, src), np_ref = __shfl (p_ref, src);
      const long nc_alt = max (o.alt_len - (long) o.phase, 0l) / 3;
      long first_diff = -1, alt_stop = -1;
      // codons [0, first) are the same bases in both: a reference that stops among them is the alternative too
      if (np_ref <= first && __shfl (r.flags, src) != 0) alt_stop = np_ref - 1;   // (flags: so far the REF_STOP bit alone)
      else
        for (long at = first; at < nc_alt; at += 64) {
          const long cdn = at + lane;
          u32 a = 0, b = 0;
          if (cdn < nc_alt) a = alt_symbol (o, tab, cdn);
          if (cdn < np_ref) b = ref_symbol (o, tab, cdn);
          const u64 stops = __ballot (a == (u32) '*');
          const u64 diffs = __ballot (cdn < nc_alt && cdn < np_ref && a != b);
          const int s = stops ? __ffsll ((long long) stops) - 1 : 64, d = diffs ? __ffsll ((long long) diffs) - 1 : 64;
          if (first_diff < 0 && d <= s && d < 64) first_diff = at + d;
          if (s < 64) { alt_stop = at + s; break; }
        }
      const long np_alt = alt_stop >= 0 ? alt_stop + 1 : nc_alt;
      if (first_diff < 0 && np_alt != np_ref) first_diff = min (np_alt, np_ref);
      u64 wr = 0, wa = 0;                                // lanes 0 to 7 translate the two windows
      if (first_diff >= 0 && lane < 8) {
        const long cdn = first_diff + lane;
        if (cdn < np_ref) wr = (u64) ref_symbol (o, tab, cdn) << (8 * lane);
        if (cdn < np_alt) wa = (u64) alt_symbol (o, tab, cdn) << (8 * lane);
      }
      for (int x = 1; x < 8; x <<= 1) { wr |= __shfl_xor (wr, x); wa |= __shfl_xor (wa, x); }
      wr = __shfl (wr, 0); wa = __shfl (wa, 0);
      if (lane == src) {
        r.first_diff = (int) first_diff;
        r.cls = first_diff < 0 ? TJAMD_EFFECT_IDENTICAL : delta == 0 ? TJAMD_EFFECT_INFRAME : TJAMD_EFFECT_FRAMESHIFT;
        r.alt_aa_len = (int) (alt_stop >= 0 ? alt_stop : nc_alt);
        if (alt_stop >= 0) r.flags |= TJAMD_EFFECT_ALT_STOP;
        r.ref_aa = wr; r.alt_aa = wa;
        out[i] = r;
      }
    }
  }
}

extern "C" long tjamd_variant_effects (tjamd_counter *c, const tjamd_coding *cod, const tjamd_variant *d_variants, long n,
                                       const tjamd_tract_feature *d_tract_feat, long n_tracts, tjamd_effect *d_out)
{
  static const char *fn = "tjamd_variant_effects";
  auto refused = [&] () -> int {                        // the checks that read no handle, the counter's device last
    if (n < 0) return set_err (TJAMD_ERR_ARG, "%s: n %ld < 0", fn, n);
    if (n >= (1l << 31)) return set_err (TJAMD_ERR_CAPACITY, "%s: %ld records", fn, n);
    if (n > 0 && (!d_variants || !d_out)) return set_err (TJAMD_ERR_ARG, "%s: null variant or output buffer", fn);
    if (d_tract_feat && n_tracts < 0) return set_err (TJAMD_ERR_ARG, "%s: n_tracts %ld < 0", fn, n_tracts);
    if (!c || !cod) return set_err (TJAMD_ERR_ARG, "%s: null counter or coding table", fn);
    if (tjamd_device_count () <= 0) return set_err (TJAMD_ERR_NO_DEVICE, "%s: TJAMD_ERR_NO_DEVICE: no HIP device visible (the records are classified on the device; no CPU fallback)", fn);
    return on_counter_device (fn, "coding table", cod->device, c);
  };
  int rc = refused ();
  Stage st (c, T_VARIANT_EFFECTS);                      // (a refused call leaves no timing behind)
  if (rc) return -rc;
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  if (n == 0) return 0;
  int *err;
  rc = flags_alone (c, fn, err);
  if (rc) return -rc;
  st.begin ();
  hipLaunchKernelGGL (variant_effects_check_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const u32 *) cod->cstart, cod->n_contigs, cod->n_features,
                      (const Variant *) d_variants, n, (const TractFeature *) d_tract_feat, n_tracts, err);
  hipLaunchKernelGGL (variant_effects_kernel, dim3 ((unsigned) std::min<long> ((n + 255) / 256, 65536)), dim3 (256), 0, c->stream, (const uint8_t *) cod->codes,
                      (const u32 *) cod->cstart, cod->n_contigs, (const CodRow *) cod->rows, cod->n_features, (const Variant *) d_variants, n,
                      (const TractFeature *) d_tract_feat, n_tracts, (Effect *) d_out, err);
  st.end ();
  int h_err = 0;
  rc = read_back (c, fn, err, &h_err, 1);
  if (rc) return -rc;
  if (h_err & 1) return -set_err (TJAMD_ERR_ARG, "%s: a record's contig is outside [0, %ld)", fn, cod->n_contigs);
  if (h_err & 2) return -set_err (TJAMD_ERR_ARG, "%s: a record has pos < 1 or a REF that ends beyond its contig", fn);
  if (h_err & 4) return -set_err (TJAMD_ERR_ARG, "%s: a record's n_flank is outside 0..32", fn);
  if (h_err & 8) return -set_err (TJAMD_ERR_ARG, "%s: a record has ref_length or alt_length < 1", fn);
  if (h_err & 16) return -set_err (TJAMD_ERR_ARG, "%s: a record's tract is outside [0, %ld)", fn, n_tracts);
  if (h_err & 32) return -set_err (TJAMD_ERR_ARG, "%s: a tract's feature index is outside [-1, %ld)", fn, cod->n_features);
  st.done ();
  return n;
}
TJ_LAST_MS (tjamd_last_variant_effects_ms, T_VARIANT_EFFECTS)

// ---- N12: the per-sample variant records merged into multi-sample sites ------------------------------------------------
// The reference leaves this to its user (docs/tutorial.md, "Downstream analyses": sort | uniq over the per-sample VCF files,
// or bcftools norm / merge); the rule as built is in include/tatajuba_sites.h.  Every record of one tract has the tract's
// index entry as its anchor, so equal alleles are equal (tract, alt_length, n_flank, alt_flank) and the merge is a stable sort
// of that key with the input index as value (kv_count_kernel / kv_scatter_kernel, only the 8-bit passes the key's width
// needs), head flags against the predecessor, two scans, a segmented reduction per site and one writing pass.  Equal keys
// stay in ascending input index, so an allele's first record is its head.  Thread mapping of the reduction as in
// locate_kernel / an_paint_kernel: a lane per site walks up to MV_LANE_WALK records itself, a longer site (at most n_samples
// records, 4096) is handed to the wavefront and reduced with __shfl_xor.  Nothing is written to the caller's buffers before
// every check has been made: the writing kernels return when the error flag is up.  The flag is the only global atomic.
// DESIGN.md section 3.5, N12.

struct Site { long long flat; int tract, contig, pos, base, ref_length, min_length, n_flank, n_alleles, first_allele, n_called, first_record, pad; u64 ref_flank; };
struct Allele { int site, alt_length, n_flank, n_samples, first_record, pad; u64 alt_flank; };
static_assert (sizeof (Site) == 64 && sizeof (Site) == sizeof (tjamd_site), "site layout");
static_assert (sizeof (Allele) == 32 && sizeof (Allele) == sizeof (tjamd_allele), "allele layout");
struct MvAgg { u64 ref_flank; int n_flank, min_length, pos; u32 first_record; };   // what a site's records have in common, before anything is written

#define MV_LANE_WALK   16               // records of a site one lane walks by itself
#define MV_MAX_SAMPLES 4096
#define MV_MAX_LENGTH  1023             // alt_length has 10 bits in the key, as in the union's rows
// err bits: 1 tract, 2 sample, 4 n_flank, 8 alt_length, 16 a (tract, sample) pair twice, 32 the records of a tract disagree, 64 ref_flank
// (tjamd_merge_variants names them)

__device__ __forceinline__ int mv_nf (int n_flank) { return min (max (n_flank, 0), 32); }   // (a refused n_flank never reaches a shift)

// mode 0: the whole key in one word, (tract, alt_length : 10, n_flank : 6, alt_flank : 2k), and the record's own checks;
// mode 1: the flank word of a two-word key, and the checks; mode 2: the other word, of record val_in[j] (the order the sort
// of the flank word left).  A refused record gets key 0.  val[j] = j in modes 0 and 1.
__global__ void mv_key_kernel (const Variant *__restrict__ rec, long n, int mode, int k, int ns, long n_tracts, const u32 *__restrict__ val_in,
                               u64 *__restrict__ key, u32 *__restrict__ val, int *__restrict__ err)
{
  for (long j = blockIdx.x * (long) blockDim.x + threadIdx.x; j < n; j += (long) gridDim.x * blockDim.x) {
    const long i = mode == 2 ? (long) val_in[j] : j;
    const int tract = rec[i].tract, sample = rec[i].sample, la = rec[i].alt_length, nf = rec[i].n_flank;
    int e = 0;
    if (tract < 0 || tract >= n_tracts) e |= 1;
    if (sample < 0 || sample >= ns) e |= 2;
    if (nf < 0 || nf > k) e |= 4;
    if (la < 0 || la > MV_MAX_LENGTH) e |= 8;
    u64 kk = 0;
    if (!e) {
      const u64 fl = rec[i].alt_flank & kmask (nf);
      const u64 rest = ((u64) tract << 16) | ((u64) la << 6) | (u64) nf;
      kk = mode == 1 ? fl : mode == 2 ? rest : ((rest << (2 * k)) | fl);   // (mode 0: 2k + 16 + the tract's bits <= 64, so 2k <= 48)
    }
    key[j] = kk;
    if (mode != 2) { val[j] = (u32) j; if (e) atomicOr (err, e); }
  }
}

// the sorted records against their predecessors: where an allele and where a site begins, the sample of each (for the
// reduction's check of pairs), and err |= 32 where two records of one tract do not have the same place, base and length
__global__ void mv_head_kernel (const Variant *__restrict__ rec, const u32 *__restrict__ val, long n, u32 *__restrict__ ahead, u32 *__restrict__ shead,
                                u32 *__restrict__ smp, int *__restrict__ err)
{
  for (long j = blockIdx.x * (long) blockDim.x + threadIdx.x; j < n; j += (long) gridDim.x * blockDim.x) {
    const Variant *r = rec + val[j];
    u32 ah = 1u, sh = 1u;
    if (j > 0) {
      const Variant *p = rec + val[j - 1];
      const int nf = mv_nf (r->n_flank);
      sh = r->tract != p->tract ? 1u : 0u;
      ah = (sh || r->alt_length != p->alt_length || nf != mv_nf (p->n_flank) || ((r->alt_flank ^ p->alt_flank) & kmask (nf)) != 0ull) ? 1u : 0u;
      if (!sh && (r->flat != p->flat || r->contig != p->contig || r->base != p->base || r->ref_length != p->ref_length)) atomicOr (err, 32);
    }
    ahead[j] = ah; shead[j] = sh; smp[j] = (u32) r->sample;
  }
}

// where allele a and site s begin in the sorted order, with the end behind the last of each
__global__ void mv_start_kernel (long n, const u32 *__restrict__ ahead, const u32 *__restrict__ aex, const u32 *__restrict__ shead, const u32 *__restrict__ sex,
                                 u32 *__restrict__ astart, u32 *__restrict__ sstart)
{
  for (long j = blockIdx.x * (long) blockDim.x + threadIdx.x; j < n; j += (long) gridDim.x * blockDim.x) {
    if (ahead[j]) astart[aex[j]] = (u32) j;
    if (shead[j]) sstart[sex[j]] = (u32) j;
    if (j == n - 1) { astart[aex[j] + ahead[j]] = (u32) n; sstart[sex[j] + shead[j]] = (u32) n; }
  }
}

// per site: F = the largest n_flank and the ref_flank of a record that has it (the largest of them: they are equal, or the
// call is refused), the smallest alt_length, pos and input index; then every record against them: err |= 64 for a ref_flank
// that differs on the record's own bases, err |= 16 for a sample that comes twice.
__global__ __launch_bounds__ (256)
void mv_site_kernel (const Variant *__restrict__ rec, const u32 *__restrict__ val, const u32 *__restrict__ smp, const u32 *__restrict__ sstart,
                     const u32 *__restrict__ tot, int ns, MvAgg *__restrict__ agg, int *__restrict__ err)
{
  __shared__ u32 seen[4][MV_MAX_SAMPLES / 32];          // per wavefront: the samples of the site it is walking
  if (__any (*(volatile int *) err != 0)) return;       // (a refused sample never reaches `seen`)
  const long n_sites = tot[1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long n_threads = (long) gridDim.x * blockDim.x;
  for (long s0 = blockIdx.x * (long) blockDim.x + wave * 64; s0 < n_sites; s0 += n_threads) {   // (uniform across a wavefront)
    const long s = s0 + lane;
    const bool have = s < n_sites;
    u32 b = 0, e = 0;
    if (have) { b = sstart[s]; e = sstart[s + 1]; }
    const bool crowded = have && (long) e - (long) b > (long) ns;   // more records than samples: one of them comes twice
    const bool wide = have && !crowded && e - b > (u32) MV_LANE_WALK;
    if (have && !crowded && !wide) {
      int F = -1, ml = 0x7fffffff, ps = 0x7fffffff, bad = 0;
      u32 fr = ~0u;
      u64 fl = 0;
      for (u32 j = b; j < e; j++) {
        const u32 i = val[j];
        const int nf = mv_nf (rec[i].n_flank);
        const u64 f = rec[i].ref_flank & kmask (nf);
        if (nf > F || (nf == F && f > fl)) { F = nf; fl = f; }
        ml = min (ml, rec[i].alt_length); ps = min (ps, rec[i].pos); fr = min (fr, i);
      }
      for (u32 j = b; j < e; j++) {
        const u32 i = val[j];
        if (((rec[i].ref_flank ^ fl) & kmask (mv_nf (rec[i].n_flank))) != 0ull) bad |= 64;
        for (u32 j2 = b; j2 < j; j2++) if (smp[j2] == smp[j]) bad |= 16;
      }
      if (bad) atomicOr (err, bad);
      const MvAgg g = {fl, F, min (ml, rec[val[b]].ref_length), ps, fr};
      agg[s] = g;
    }
    if (crowded) atomicOr (err, 16);
    u64 todo = __ballot (wide);
    while (todo) {                                      // the wide sites of these 64, one after the other, all lanes on each
      const int src = __ffsll ((long long) todo) - 1;
      todo &= todo - 1ull;
      const u32 wb = __shfl (b, src), we = __shfl (e, src);
      int F = -1, ml = 0x7fffffff, ps = 0x7fffffff, bad = 0;
      u32 fr = ~0u;
      u64 fl = 0;
      for (u32 j = wb + lane; j < we; j += 64) {
        const u32 i = val[j];
        const int nf = mv_nf (rec[i].n_flank);
        const u64 f = rec[i].ref_flank & kmask (nf);
        if (nf > F || (nf == F && f > fl)) { F = nf; fl = f; }
        ml = min (ml, rec[i].alt_length); ps = min (ps, rec[i].pos); fr = min (fr, i);
      }
      for (int o = 32; o; o >>= 1) {
        const int F2 = __shfl_xor (F, o);
        const u64 fl2 = shfl_xor64 (fl, o);
        if (F2 > F || (F2 == F && fl2 > fl)) { F = F2; fl = fl2; }
        ml = min (ml, __shfl_xor (ml, o)); ps = min (ps, __shfl_xor (ps, o)); fr = min (fr, __shfl_xor (fr, o));
      }
      seen[wave][lane] = 0u; seen[wave][lane + 64] = 0u;
      __threadfence_block ();                           // (one wavefront: its LDS operations keep their order; the fence keeps the compiler's)
      for (u32 j = wb + lane; j < we; j += 64) {
        const u32 i = val[j], sm = smp[j];
        if (((rec[i].ref_flank ^ fl) & kmask (mv_nf (rec[i].n_flank))) != 0ull) bad |= 64;
        if (sm < (u32) ns && (atomicOr (&seen[wave][sm >> 5], 1u << (sm & 31u)) & (1u << (sm & 31u)))) bad |= 16;
      }
      __threadfence_block ();
      if (bad) atomicOr (err, bad);
      if (lane == 0) {
        const MvAgg g = {fl, F, min (ml, rec[val[wb]].ref_length), ps, fr};
        agg[s0 + src] = g;
      }
    }
  }
}

// the genotype rows of the sites found, those below the capacity: no record
__global__ void mv_fill_kernel (const u32 *__restrict__ tot, long site_cap, int ns, int16_t *__restrict__ gt, const int *__restrict__ err)
{
  if (*err) return;
  const long cells = min ((long) tot[1], site_cap) * (long) ns;
  for (long x = blockIdx.x * (long) blockDim.x + threadIdx.x; x < cells; x += (long) gridDim.x * blockDim.x) gt[x] = (int16_t) -1;
}

// one thread per sorted record: its allele index and genotype cell; an allele's head writes the allele and its record, a
// site's head the site.  Nothing at or beyond a capacity.
__global__ void mv_write_kernel (const Variant *__restrict__ rec, const u32 *__restrict__ val, long n, int ns, const u32 *__restrict__ ahead, const u32 *__restrict__ aex,
                                 const u32 *__restrict__ shead, const u32 *__restrict__ sex, const u32 *__restrict__ astart, const u32 *__restrict__ sstart,
                                 const MvAgg *__restrict__ agg, const u32 *__restrict__ tot, Site *__restrict__ sites, long site_cap, Allele *__restrict__ alleles, long allele_cap,
                                 int16_t *__restrict__ gt, int *__restrict__ allele_of, Variant *__restrict__ unique, const int *__restrict__ err)
{
  if (*err) return;
  const u32 n_alleles = tot[0];
  for (long j = blockIdx.x * (long) blockDim.x + threadIdx.x; j < n; j += (long) gridDim.x * blockDim.x) {
    const u32 i = val[j];
    const Variant r = rec[i];
    const u32 a = aex[j] + ahead[j] - 1u, s = sex[j] + shead[j] - 1u;
    const u32 sb = sstart[s], a0 = aex[sb];             // (a site's head is an allele's head: the alleles in front of it are its number)
    const MvAgg g = agg[s];
    if (allele_of) allele_of[i] = (int) a;
    if (gt && (long) s < site_cap) gt[(long) s * ns + r.sample] = (int16_t) (a - a0 + 1u);
    if (ahead[j] && (long) a < allele_cap) {
      const u64 own = kmask (mv_nf (r.n_flank));          // (k = 32: kmask, not a shift by 64)
      Allele o;
      o.site = (int) s; o.alt_length = r.alt_length; o.n_flank = r.n_flank; o.n_samples = (int) (astart[a + 1] - (u32) j); o.first_record = (int) i; o.pad = 0;
      o.alt_flank = (r.alt_flank & own) | (g.ref_flank & ~own);
      alleles[a] = o;
      if (unique) unique[a] = r;
    }
    if (shead[j] && (long) s < site_cap) {
      const u32 se = sstart[s + 1], a1 = (long) se < n ? aex[se] : n_alleles;
      Site o;
      o.flat = r.flat; o.tract = r.tract; o.contig = r.contig; o.pos = g.pos; o.base = r.base; o.ref_length = r.ref_length; o.min_length = g.min_length;
      o.n_flank = g.n_flank; o.n_alleles = (int) (a1 - a0); o.first_allele = (int) a0; o.n_called = (int) (se - sb); o.first_record = (int) g.first_record; o.pad = 0;
      o.ref_flank = g.ref_flank;
      sites[s] = o;
    }
  }
}

static int mv_tract_bits (long n_tracts) { int b = 0; while (b < 31 && (1l << b) < n_tracts) b++; return b; }   // the bits of tract ids below n_tracts

extern "C" long tjamd_merge_variants (tjamd_counter *c, int kmer_size, const tjamd_variant *d_records, long n_records, int n_samples, long n_tracts,
                                      tjamd_site *d_sites, long site_capacity, tjamd_allele *d_alleles, long allele_capacity,
                                      int16_t *d_genotype, int *d_allele_of, tjamd_variant *d_unique, long *h_n_alleles)
{
  static const char *fn = "tjamd_merge_variants";
  const long n = n_records;
  auto refused = [&] () -> int {                        // the checks that read no handle, the device last
    if (!c) return set_err (TJAMD_ERR_ARG, "%s: null counter", fn);
    if (n < 0 || n >= (1l << 31)) return set_err (TJAMD_ERR_ARG, "%s: n_records %ld outside 0..2^31-1", fn, n);
    if (n_samples < 1 || n_samples > MV_MAX_SAMPLES) return set_err (TJAMD_ERR_ARG, "%s: n_samples %d outside 1..4096", fn, n_samples);
    if (kmer_size < 2 || kmer_size > 32) return set_err (TJAMD_ERR_ARG, "%s: kmer_size %d outside [2,32]", fn, kmer_size);
    if (n_tracts < 0) return set_err (TJAMD_ERR_ARG, "%s: n_tracts %ld < 0", fn, n_tracts);
    if (site_capacity < 0 || allele_capacity < 0) return set_err (TJAMD_ERR_ARG, "%s: capacities %ld and %ld", fn, site_capacity, allele_capacity);
    if (n > 0 && !d_records) return set_err (TJAMD_ERR_ARG, "%s: null record buffer", fn);
    if ((site_capacity > 0 && !d_sites) || (allele_capacity > 0 && !d_alleles)) return set_err (TJAMD_ERR_ARG, "%s: null site or allele buffer", fn);
    if (!h_n_alleles) return set_err (TJAMD_ERR_ARG, "%s: null h_n_alleles", fn);
    if (tjamd_device_count () <= 0) return set_err (TJAMD_ERR_NO_DEVICE, "%s: TJAMD_ERR_NO_DEVICE: no HIP device visible (the records are merged on the device; no CPU fallback)", fn);
    return TJAMD_OK;
  };
  int rc = refused ();
  Stage st (c, T_MERGE_VARIANTS);                       // (a refused call leaves no timing behind)
  if (rc) return -rc;
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  if (n == 0) { *h_n_alleles = 0; return 0; }
  const int k = kmer_size, tbits = mv_tract_bits (n_tracts);
  const bool one_word = tbits + 16 + 2 * k <= 64;
  ScratchCut cut;
  u64 *key[2]; u32 *val[2], *ahead, *shead, *aex, *sex, *smp, *astart, *sstart, *tot; MvAgg *agg;
  cut.take (key[0], n); cut.take (key[1], n); cut.take (val[0], n); cut.take (val[1], n);
  cut.take (ahead, n); cut.take (shead, n); cut.take (aex, n); cut.take (sex, n); cut.take (smp, n);
  cut.take (astart, (size_t) n + 1); cut.take (sstart, (size_t) n + 1); cut.take (agg, n); cut.take (tot, 64);
  rc = cut.commit (c);
  if (!rc) rc = reserve_sort (c, n, n);
  if (rc) return -rc;
  int *err = (int *) tot + 2;                           // tot: the alleles, the sites, the error flag
  if (hipMemsetAsync (tot, 0, 256, c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: memset failed", fn);
  st.begin ();
  const Variant *rec = (const Variant *) d_records;
  const unsigned grid = grid_for (n);
  if (one_word) {
    hipLaunchKernelGGL (mv_key_kernel, dim3 (grid), dim3 (256), 0, c->stream, rec, n, 0, k, n_samples, n_tracts, (const u32 *) nullptr, key[0], val[0], err);
    rc = kv_sort (c, key, val, n, tbits + 16 + 2 * k);
  } else {                                              // the flank word first, then the rest: the second sort keeps the first one's order
    hipLaunchKernelGGL (mv_key_kernel, dim3 (grid), dim3 (256), 0, c->stream, rec, n, 1, k, n_samples, n_tracts, (const u32 *) nullptr, key[0], val[0], err);
    rc = kv_sort (c, key, val, n, 2 * k);
    if (!rc) {
      hipLaunchKernelGGL (mv_key_kernel, dim3 (grid), dim3 (256), 0, c->stream, rec, n, 2, k, n_samples, n_tracts, (const u32 *) val[0], key[0], (u32 *) nullptr, err);
      rc = kv_sort (c, key, val, n, tbits + 16);
    }
  }
  if (rc) return -rc;
  hipLaunchKernelGGL (mv_head_kernel, dim3 (grid), dim3 (256), 0, c->stream, rec, (const u32 *) val[0], n, ahead, shead, smp, err);
  rc = exclusive_scan (c, ahead, aex, n, tot);
  if (!rc) rc = exclusive_scan (c, shead, sex, n, tot + 1);
  if (rc) return -rc;
  hipLaunchKernelGGL (mv_start_kernel, dim3 (grid), dim3 (256), 0, c->stream, n, (const u32 *) ahead, (const u32 *) aex, (const u32 *) shead, (const u32 *) sex, astart, sstart);
  hipLaunchKernelGGL (mv_site_kernel, dim3 (grid), dim3 (256), 0, c->stream, rec, (const u32 *) val[0], (const u32 *) smp, (const u32 *) sstart, (const u32 *) tot, n_samples, agg, err);
  if (d_genotype)
    hipLaunchKernelGGL (mv_fill_kernel, dim3 (grid_for (std::min (n, site_capacity) * (long) n_samples)), dim3 (256), 0, c->stream, (const u32 *) tot, site_capacity, n_samples,
                        d_genotype, (const int *) err);
  hipLaunchKernelGGL (mv_write_kernel, dim3 (grid), dim3 (256), 0, c->stream, rec, (const u32 *) val[0], n, n_samples, (const u32 *) ahead, (const u32 *) aex,
                      (const u32 *) shead, (const u32 *) sex, (const u32 *) astart, (const u32 *) sstart, (const MvAgg *) agg, (const u32 *) tot,
                      (Site *) d_sites, site_capacity, (Allele *) d_alleles, allele_capacity, d_genotype, d_allele_of, (Variant *) d_unique, (const int *) err);
  st.end ();
  u32 h[3] = {0, 0, 0};
  rc = read_back (c, fn, tot, h, 3);
  if (rc) return -rc;
  if (h[2] & 1u) return -set_err (TJAMD_ERR_ARG, "%s: a record's tract is outside [0, %ld)", fn, n_tracts);
  if (h[2] & 2u) return -set_err (TJAMD_ERR_ARG, "%s: a record's sample is outside [0, %d)", fn, n_samples);
  if (h[2] & 4u) return -set_err (TJAMD_ERR_ARG, "%s: a record's n_flank is outside 0..%d", fn, k);
  if (h[2] & 8u) return -set_err (TJAMD_ERR_ARG, "%s: a record's alt_length is outside 0..%d", fn, MV_MAX_LENGTH);
  if (h[2] & 32u) return -set_err (TJAMD_ERR_ARG, "%s: records of one tract disagree in flat, contig, base or ref_length", fn);
  if (h[2] & 16u) return -set_err (TJAMD_ERR_ARG, "%s: a (tract, sample) pair occurs twice", fn);
  if (h[2] & 64u) return -set_err (TJAMD_ERR_ARG, "%s: records of one tract disagree in ref_flank on their own n_flank bases", fn);
  if ((long) h[1] > site_capacity || (long) h[0] > allele_capacity)
    return -set_err (TJAMD_ERR_CAPACITY, "%s: %u sites and %u alleles, caller capacities %ld and %ld", fn, h[1], h[0], site_capacity, allele_capacity);
  *h_n_alleles = (long) h[0];
  st.done ();
  return (long) h[1];
}
TJ_LAST_MS (tjamd_last_merge_variants_ms, T_MERGE_VARIANTS)

// ---- N13: per-site read depths and reference genotypes of the merged sites ------------------------------------------------
// What tjamd_merge_variants cannot know from N8's records: whether a sample without a record equals the reference or has no
// read on the tract.  The count matrix of the union tells; the rule as built is in include/tatajuba_depths.h.  Segment mapping
// of tract_variants_kernel: S lanes per site, a lane per sample (looping beyond 64), a count row read as S consecutive words;
// what the samples share -- the tract's rows (tract_rows), its index entry and k_eff (located_tract), the site's allele range -- is
// found by the segment's first lane and broadcast.  A row's class (REF, an allele of the site, OTHER) does not depend on the sample:
// the lanes of a segment classify a chunk of S rows, one row each (row_right_flank, the rule N8's records were written by, then
// the search among the site's alleles), and then every lane walks the chunk for its own sample and takes each row's class with
// __shfl.  DP, the modal row with its class and length, and eight class accumulators (REF and seven alleles; selected by
// unrolled compares, nothing indexed, nothing in scratch memory) stay in registers; a site with more than eight classes walks
// its rows once more per further eight.  Two passes of one kernel: the first makes every check, leaves what a site's samples
// share in scratch and writes nothing else, the second returns while the flag is up and reads neither tiling nor sites again.  DESIGN.md section 3.5, N13.

struct SiteDepth { int n_ref, n_missing; long long depth; };
static_assert (sizeof (SiteDepth) == 16 && sizeof (SiteDepth) == sizeof (tjamd_site_depth), "site depth layout");
struct SdShared { int first, end, k_eff, a0, na, Lr, neg, ok; u64 fr; };   // what the samples of a site share, from the first pass to the second

#define SD_GROUP 8                      // class accumulators of one walk
// err bits: 1 tiling, 2 site.tract, 4 the site against its tract's location and entry, 8 the allele chain, 16 n_alleles < 1,
// 32 allele.site, 64 allele.n_flank, 128 a modal row that no allele holds, 256 n_called (tjamd_site_depths names them)

// The allele chain of the merged sites, the rule of N13's first pass and of N14's check: bit 16 where site i (first_allele a0,
// n_alleles na) has no allele, bit 8 where it does not begin where site i - 1 ends (the first: at 0) or, the last one, does not end
// at n_alleles.  site_bit_refused: the text of either bit and of bit 32 (an allele outside its site; each entry finds that in its
// own way), one bit per call, so that each entry keeps its own order of decoding.
__device__ __forceinline__ int site_chain_bad (const Site *__restrict__ sites, long n_sites, long n_alleles, long i, int a0, int na)
{
  const long a_want = i ? (long) sites[i - 1].first_allele + (long) sites[i - 1].n_alleles : 0l;
  return (na < 1 ? 16 : 0) | ((long) a0 != a_want || (i == n_sites - 1 && (long) a0 + (long) na != n_alleles) ? 8 : 0);
}
static int site_bit_refused (const char *fn, u32 bit, long n_alleles)
{
  if (bit == 16u) return set_err (TJAMD_ERR_ARG, "%s: a site has n_alleles < 1", fn);
  if (bit == 8u) return set_err (TJAMD_ERR_ARG, "%s: first_allele and n_alleles of the sites do not chain from 0 to %ld", fn, n_alleles);
  return set_err (TJAMD_ERR_ARG, "%s: an allele's site is not the site that holds it", fn);
}

__device__ __forceinline__ int sd_saturated (long long x) { return x > 0x7fffffffll ? 0x7fffffff : (int) x; }

template <bool WRITE>
__global__ __launch_bounds__ (256)
void site_depths_kernel (const u64 *__restrict__ keys, const int *__restrict__ counts, long n_union, int ns, int S, int k,
                         const UnionTract *__restrict__ tracts, long n_tracts, const Location *__restrict__ tloc,
                         const RefEntry *__restrict__ entries, long n_ent, const Site *__restrict__ sites, long n_sites,
                         const Allele *__restrict__ alleles, long n_alleles, int16_t *__restrict__ gt, int *__restrict__ dp, int *__restrict__ ad,
                         SiteDepth *__restrict__ summary, SdShared *__restrict__ shared, int *__restrict__ err)
{
  const long gthread = blockIdx.x * (long) blockDim.x + threadIdx.x, n_threads = (long) gridDim.x * blockDim.x;
  if (WRITE) { if (*(volatile int *) err != 0) return; }   // (the first pass is complete: every thread reads the same word)
  else check_tiling (tracts, n_tracts, n_union, err);
  const int lane = threadIdx.x & (S - 1);
  const int log_S = __ffs (S) - 1;                       // (S is a power of two)
  const long segs_per_grid = n_threads >> log_S;         // (its own spelling, not SEGMENT_MAP's: shifts, and this kernel's code as it was)
  for (long i = gthread >> log_S; i < n_sites; i += segs_per_grid) {   // (uniform across a segment)
    int first = 0, end = 0, ent = -1, a0 = 0;           // (rows, entries and alleles are fewer than 2^31: the entry checks it)
    int k_eff = 0, na = 0, n_called = 0, Lr = 0, neg = 0;
    u64 fr = 0;                                         // the entry's length, strand and forward right flank
    if (WRITE) {                                        // (one address per segment)
      const SdShared p = shared[i];
      first = p.first; end = p.end; k_eff = p.k_eff; a0 = p.a0; na = p.na; Lr = p.Lr; neg = p.neg; fr = p.fr; ent = p.ok - 1;
    }
    else if (lane == 0) {
      const Site site = sites[i];
      const long t = site.tract;
      n_called = site.n_called;
      a0 = site.first_allele; na = site.n_alleles;
      int bad = site_chain_bad (sites, n_sites, n_alleles, i, a0, na);
      if (a0 < 0 || na < 1 || (long) a0 + (long) na > n_alleles) { if (na >= 1) bad |= 8; a0 = 0; na = 0; }   // (nothing is read outside the alleles)
      long t_first = 0, t_end = 0;
      if (t < 0 || t >= n_tracts) bad |= 2;
      else tract_rows (tracts[t], n_union, t_first, t_end);   // (none of a broken tiling: flagged above)
      first = (int) t_first; end = (int) t_end;
      if (first < end) {                                // the site is its tract's: the entry there, and what N12 copied from the records
        const Location l = tloc[t];
        ent = (int) located_tract (tloc, n_tracts, t, entries, n_ent, k, k_eff);
        if (ent < 0 || site.flat != l.flat || site.contig != l.contig || site.ref_length != entries[ent].length) { bad |= 4; ent = -1; }
      }
      if (bad) { ent = -1; atomicOr (err, bad); }
      if (ent >= 0) { const RefEntry e = entries[ent]; Lr = e.length; neg = e.neg_strand; fr = entry_right_flank (e, k); }
      const SdShared p = {first, end, k_eff, a0, na, Lr, neg, ent >= 0 ? 1 : 0, fr};
      shared[i] = p;
    }
    if (!WRITE) {
      first = __shfl (first, 0, S); end = __shfl (end, 0, S); ent = __shfl (ent, 0, S); a0 = __shfl (a0, 0, S);
      k_eff = __shfl (k_eff, 0, S); na = __shfl (na, 0, S); n_called = __shfl (n_called, 0, S); Lr = __shfl (Lr, 0, S); neg = __shfl (neg, 0, S);
      fr = shfl64 (fr, 0, S);
      int bad = 0;                                      // the site's alleles, a lane each
      for (int a = lane; a < na; a += S) {
        if (alleles[a0 + a].site != (int) i) bad |= 32;
        if (alleles[a0 + a].n_flank < 0 || alleles[a0 + a].n_flank > k) bad |= 64;
      }
      if (bad) atomicOr (err, bad);
    }
    if (ent < 0) continue;                              // (refused; uniform across the segment)
    const int n_groups = WRITE && ad ? (na + 1 + SD_GROUP - 1) / SD_GROUP : 1;
    int n_ref = 0, n_missing = 0, n_alt = 0;
    long long depth = 0;
    for (int s0 = 0; s0 < ns; s0 += S) {                // (every lane of the segment stays in the loop: the shuffles need them)
      const int s = s0 + lane;
      const bool mine = s < ns;
      for (int grp = 0; grp < n_groups; grp++) {
        const int c0 = grp * SD_GROUP;                  // the classes of this walk: [c0, c0 + SD_GROUP)
        long long sum = 0, acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0, acc4 = 0, acc5 = 0, acc6 = 0, acc7 = 0;
        int best = 0, m_cls = -1, m_la = 0;
        for (int base = first, n_here; base < end; base += n_here) {      // a chunk of S rows (no sum beyond `end`: it may be near 2^31)
          const long r_own = (long) base + lane;
          n_here = min (S, end - base);
          int cls = -1, la = 0;                         // this lane's row of the chunk
          if (r_own < end) {
            la = meta_len (keys[3 * r_own + 2]);
            if (la == Lr && la >= 1) cls = 0;
            else if (la >= 1) {
              int nf;
              const u64 fa = row_right_flank (keys, r_own, neg, k, k_eff, fr, nf);
              #pragma unroll 1
              for (int a = 0; a < na; a++) {
                const Allele al = alleles[a0 + a];
                if (al.alt_length == la && al.n_flank == nf && ((al.alt_flank ^ fa) & kmask (nf)) == 0ull) { cls = a + 1; break; }
              }
            }
          }
          #pragma unroll 1
          for (int r = 0; r < n_here; r++) {
            const int c = __shfl (cls, r, S), l = __shfl (la, r, S);
            const int x = mine ? max (counts[(long) (base + r) * ns + s], 0) : 0;   // (counts <= 0 contribute nothing)
            const int g = c - c0;
            const bool better = x > best;               // (the first on a tie)
            sum += x;
            best = better ? x : best; m_cls = better ? c : m_cls; m_la = better ? l : m_la;
            acc0 += g == 0 ? x : 0; acc1 += g == 1 ? x : 0; acc2 += g == 2 ? x : 0; acc3 += g == 3 ? x : 0;
            acc4 += g == 4 ? x : 0; acc5 += g == 5 ? x : 0; acc6 += g == 6 ? x : 0; acc7 += g == 7 ? x : 0;
          }
        }
        if (grp == 0 && mine) {
          int g = -1;
          if (best > 0 && m_la >= 1) {
            if (m_cls >= 0) g = m_cls;
            else if (!WRITE) atomicOr (err, 128);       // N8 has a record here that the alleles do not hold
          }
          n_ref += g == 0; n_missing += g < 0; n_alt += g > 0; depth += sum;
          if (WRITE) {
            if (gt) gt[i * ns + s] = (int16_t) g;
            if (dp) dp[i * ns + s] = sd_saturated (sum);
          }
        }
        if (WRITE && ad && mine) {
          int *row = ad + ((long) a0 + i + c0) * ns + s;
          const int left = na + 1 - c0;                 // the classes from c0 on
          if (left > 0) row[0] = sd_saturated (acc0);
          if (left > 1) row[(long) ns] = sd_saturated (acc1);
          if (left > 2) row[2l * ns] = sd_saturated (acc2);
          if (left > 3) row[3l * ns] = sd_saturated (acc3);
          if (left > 4) row[4l * ns] = sd_saturated (acc4);
          if (left > 5) row[5l * ns] = sd_saturated (acc5);
          if (left > 6) row[6l * ns] = sd_saturated (acc6);
          if (left > 7) row[7l * ns] = sd_saturated (acc7);
        }
      }
    }
    for (int o = S >> 1; o; o >>= 1) {
      n_ref += __shfl_xor (n_ref, o, S); n_missing += __shfl_xor (n_missing, o, S); n_alt += __shfl_xor (n_alt, o, S);
      depth += (long long) shfl_xor64 ((u64) depth, o, S);
    }
    if (lane == 0) {
      if (!WRITE) { if (n_alt != n_called) atomicOr (err, 256); }
      else if (summary) { const SiteDepth o = {n_ref, n_missing, depth}; summary[i] = o; }
    }
  }
}

extern "C" long tjamd_site_depths (tjamd_counter *c, const tjamd_reference *ref, const void *d_keys, const void *d_counts, long n_union, int n_samples,
                                   const tjamd_union_tract *d_tracts, long n_tracts, const tjamd_location *d_tract_loc,
                                   const tjamd_site *d_sites, long n_sites, const tjamd_allele *d_alleles, long n_alleles,
                                   int16_t *d_genotype, int *d_depth, int *d_allele_depth, tjamd_site_depth *d_summary)
{
  static const char *fn = "tjamd_site_depths";
  if (!c || !ref) return -set_err (TJAMD_ERR_ARG, "%s: null counter or reference", fn);
  int rc = tiled_union_args (fn, d_keys, d_counts, n_union, n_samples, d_tracts, n_tracts, d_tract_loc);
  if (rc) return -rc;
  if (n_sites < 0 || n_alleles < 0) return -set_err (TJAMD_ERR_ARG, "%s: n_sites %ld, n_alleles %ld: a count below 0", fn, n_sites, n_alleles);
  if ((n_sites > 0 && !d_sites) || (n_alleles > 0 && !d_alleles)) return -set_err (TJAMD_ERR_ARG, "%s: null site or allele buffer", fn);
  if (n_sites > n_tracts) return -set_err (TJAMD_ERR_ARG, "%s: %ld sites for %ld tracts", fn, n_sites, n_tracts);
  if (n_alleles < n_sites) return -set_err (TJAMD_ERR_ARG, "%s: %ld alleles for %ld sites (a site has at least one)", fn, n_alleles, n_sites);
  if (n_alleles >= (1l << 31) || (n_sites + n_alleles) * (long) n_samples >= (1l << 31))
    return -set_err (TJAMD_ERR_ARG, "%s: (%ld sites + %ld alleles) x %d samples: 2^31 cells or more", fn, n_sites, n_alleles, n_samples);
  if (tjamd_device_count () <= 0) return -set_err (TJAMD_ERR_NO_DEVICE, "%s: TJAMD_ERR_NO_DEVICE: no HIP device visible (the depths are counted on the device; no CPU fallback)", fn);
  if (ref->n_entries >= (1l << 31)) return -set_err (TJAMD_ERR_CAPACITY, "%s: %ld index entries", fn, ref->n_entries);
  Stage st (c, T_SITE_DEPTHS);                          // (a refused call leaves no timing behind)
  if (const int bad = reference_of_counter (fn, ref, c)) return -bad;
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  if (n_sites == 0) return 0;
  ScratchCut cut;
  int *err; SdShared *shared;
  cut.take (err, 64); cut.take (shared, (size_t) n_sites);
  rc = cut.commit (c);
  if (rc) return -rc;
  if (hipMemsetAsync (err, 0, 256, c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: memset failed", fn);
  st.begin ();
  const int S = tract_segment (n_samples);
  auto launch = [&] (auto kernel) {
    hipLaunchKernelGGL (kernel, dim3 (tract_grid (n_sites, S)), dim3 (256), 0, c->stream, (const u64 *) d_keys, (const int *) d_counts, n_union, n_samples, S, c->k,
                        (const UnionTract *) d_tracts, n_tracts, (const Location *) d_tract_loc, (const RefEntry *) ref->entries, ref->n_entries,
                        (const Site *) d_sites, n_sites, (const Allele *) d_alleles, n_alleles, d_genotype, d_depth, d_allele_depth, (SiteDepth *) d_summary, shared, err);
  };
  launch (site_depths_kernel<false>);                   // every check; nothing of the caller's is written
  launch (site_depths_kernel<true>);                    // returns while the flag is up
  st.end ();
  u32 h_err = 0;
  rc = read_back (c, fn, err, &h_err, 1);
  if (rc) return -rc;
  if (h_err & 1u) return -set_err (TJAMD_ERR_ARG, TILING_REFUSED, fn);
  if (h_err & 2u) return -set_err (TJAMD_ERR_ARG, "%s: a site's tract is outside [0, %ld)", fn, n_tracts);
  if (h_err & 16u) return -site_bit_refused (fn, 16u, n_alleles);
  if (h_err & 8u) return -site_bit_refused (fn, 8u, n_alleles);
  if (h_err & 4u) return -set_err (TJAMD_ERR_ARG, "%s: a site has no index entry, or its flat, contig or ref_length is not its tract's", fn);
  if (h_err & 32u) return -site_bit_refused (fn, 32u, n_alleles);
  if (h_err & 64u) return -set_err (TJAMD_ERR_ARG, "%s: an allele's n_flank is outside 0..%d", fn, c->k);
  if (h_err & 128u) return -set_err (TJAMD_ERR_ARG, "%s: a sample's modal row is a variant that the site's alleles do not hold (sites of another union or list)", fn);
  if (h_err & 256u) return -set_err (TJAMD_ERR_ARG, "%s: a site's n_called is not the number of samples with an allele (sites merged from another list or a subset)", fn);
  st.done ();
  return n_sites;
}
TJ_LAST_MS (tjamd_last_site_depths_ms, T_SITE_DEPTHS)

// ---- N14: pairwise sample distances over the merged sites -------------------------------------------------------------------
// The site x sample genotype matrix of N12 / N13 reduced to a sample x sample matrix of (n_both, n_differ, length_diff); the rule
// as built is in include/tatajuba_distances.h.  The first step since the scan whose cost is arithmetic: S^2 T / 2 cell pairs.
// A workgroup owns a tile of E x E sample pairs on or above the diagonal and a slice of the sites.  Per chunk of SDIST_CELLS / E
// sites it stages the genotypes of its two sample tiles into LDS and, beside each, the cell's length (ref_length or the allele's
// alt_length), which the check pass has looked up once per cell and left in scratch, an int per cell (looked up while staging,
// by every tile that stages the cell, the gather of 32-byte alleles took more time than the arithmetic at 1024 samples); then
// every thread walks the chunk's sites for a register block of 4 x 4 pairs, reading four cells
// of either tile as one 16-byte LDS load.  E is 64 where the tile pairs alone fill the device (16 x 16 threads, every thread
// walks every site) and 32, 16 or 8 below (8 x 8, 4 x 4, 2 x 2 pair threads, and the 4, 16 or 64 thread groups that this leaves
// take every 4th, 16th or 64th site of the chunk; their sums meet in LDS atomics at the end of the workgroup).  A pair of cells costs six vector
// instructions and no branch: the AND of the two cells' called masks (made once per cell), n_both minus that mask, a compare
// and a carry-add for the equal calls, a bit select and one v_sad_u32 that adds |La - Lb| to a 32-bit sum; the 32-bit sums are flushed into 64-bit ones before they can overflow (the
// bound is the chunk's largest staged length: see the kernel).  Where the sites are split over workgroups (few tile pairs) every workgroup stores its
// tile in scratch and a third kernel sums the slices in their order; otherwise a tile is stored at once.  No atomic reaches
// global memory but the error flag's (device-wide atomics on the matrix, tried first, took more time than the arithmetic at 1024
// samples).  Off-diagonal tiles are written to both halves.  Two or three kernels; the first makes every check and writes
// nothing of the caller's, the others return while the flag is up.
// DESIGN.md section 3.5, N14.

struct SampleDistance { int n_both, n_differ; long long length_diff; };
static_assert (sizeof (SampleDistance) == 16 && sizeof (SampleDistance) == sizeof (tjamd_sample_distance), "sample distance layout");

#define SDIST_CELLS 2048                // cells of one sample tile in a chunk: E samples x SDIST_CELLS / E sites (4 arrays of ints: 32 KB of LDS)
// err bits: 1 a genotype cell, 8 the allele chain, 16 n_alleles < 1, 32 allele.site, 64 alt_length, 128 ref_length (tjamd_sample_distances names them)

__global__ __launch_bounds__ (256)
void sample_distances_check_kernel (const Site *__restrict__ sites, long n_sites, const Allele *__restrict__ alleles, long n_alleles,
                                    const int16_t *__restrict__ gt, int ns, int *__restrict__ lens, int *__restrict__ err)
{
  const long gthread = blockIdx.x * (long) blockDim.x + threadIdx.x, n_threads = (long) gridDim.x * blockDim.x;
  int bad = 0;
  for (long i = gthread; i < n_sites; i += n_threads) {
    bad |= site_chain_bad (sites, n_sites, n_alleles, i, sites[i].first_allele, sites[i].n_alleles);
    if (sites[i].ref_length < 0) bad |= 128;
  }
  for (long a = gthread; a < n_alleles; a += n_threads) {   // (where the chain holds, an allele lies in one site's range: its own)
    const long s = alleles[a].site;
    const int len = alleles[a].alt_length;
    if (s < 0 || s >= n_sites || a < (long) sites[s].first_allele || a >= (long) sites[s].first_allele + (long) sites[s].n_alleles) bad |= 32;
    if (len < 0 || len > 1023) bad |= 64;
  }
  const int n_cells = (int) (n_sites * ns);             // (below 2^31: the entry checks it)
  for (long x = gthread; x < n_cells; x += n_threads) {   // every cell's length, looked up here once and not by every tile that stages the cell
    const int g = gt[x], site = (int) x / ns;
    int len = 0;
    if (g < -1 || g > sites[site].n_alleles) bad |= 1;
    else if (g == 0) len = sites[site].ref_length;
    else if (g > 0) {
      const long a = (long) sites[site].first_allele + g - 1;
      if (a >= 0 && a < n_alleles) len = alleles[a].alt_length;   // (otherwise the chain is broken: flagged above)
    }
    lens[x] = len;                                      // (scratch)
  }
  if (bad) atomicOr (err, bad);
}

// a pair's sums into the matrix, and into its other half for a pair of an off-diagonal tile
__device__ __forceinline__ void sdist_emit (SampleDistance *__restrict__ out, int ns, int a, int b, bool mirror, const SampleDistance &o)
{
  if (a >= ns || b >= ns) return;
  out[(long) a * ns + b] = o;
  if (mirror) out[(long) b * ns + a] = o;
}

// the tile pair (ti <= tj) with number p: row ti of the upper triangle has n_tiles - ti of them
__device__ __forceinline__ void sdist_tile_pair (int p, int n_tiles, int &ti, int &tj)
{
  ti = 0;
  while (p >= n_tiles - ti) { p -= n_tiles - ti; ti++; }
  tj = ti + p;
}

// Staging of one chunk (the CH = SDIST_CELLS / E sites from c0) of the two sample tiles into gA, lA, gB, lB, SDIST_CELLS / 256 cells
// of either tile a thread: a row of E samples is E consecutive int16 of the matrix and E consecutive lengths of the check pass.
// Every load is issued before anything waits for one.  A missing cell is staged as -1 in one tile and -2 in the other, so that
// two equal words are two calls of one allele; its length is 0.  A length beyond an allele's 1023 raises *l_max, the chunk's largest.
template <int E>
__device__ __forceinline__ void sdist_stage (const int16_t *__restrict__ gt, const int *__restrict__ lens, int ns, int a0, int b0, long c0, long s_end, int tid,
                                             int *gA, int *lA, int *gB, int *lB, int *l_max)
{
  int g_st[2][SDIST_CELLS / 256], len_st[2][SDIST_CELLS / 256];
  #pragma unroll
  for (int j = 0; j < SDIST_CELLS / 256; j++) {
    const int x = tid + 256 * j;
    const long site = c0 + x / E;
    #pragma unroll
    for (int h = 0; h < 2; h++) {
      const int sample = (h ? b0 : a0) + x % E;
      const bool in = site < s_end && sample < ns;
      g_st[h][j] = in ? (int) gt[site * ns + sample] : -1;
      len_st[h][j] = in ? lens[site * ns + sample] : 0;
    }
  }
  #pragma unroll
  for (int j = 0; j < SDIST_CELLS / 256; j++)
    #pragma unroll
    for (int h = 0; h < 2; h++) {
      const int x = tid + 256 * j, g = g_st[h][j], len = len_st[h][j];
      if (len > 1023) atomicMax (l_max, len);
      (h ? gB : gA)[x] = g < 0 ? -1 - h : g;
      (h ? lB : lA)[x] = len;
    }
}

// A workgroup's tile of sums, behind its last chunk, to its place: `mine` where the sites are split (the whole tile goes to this
// workgroup's place in scratch), otherwise the matrix.  With one thread group (Z == 1) a thread stores its 4 x 4 pairs; with
// several their sums meet in the staging area first (the site loop's last barrier is behind every read of it).
template <int E>
__device__ __forceinline__ void sdist_store_tile (const int (&nb)[4][4], const int (&same)[4][4], const u64 (&ld)[4][4], int *lds, SampleDistance *__restrict__ mine,
                                                  SampleDistance *__restrict__ out, int ns, int a0, int b0, bool mirror, int tid)
{
  constexpr int T = E / 4, Z = 256 / (T * T);
  const int tx = tid % T, ty = (tid / T) % T;
  if constexpr (Z == 1) {
    #pragma unroll
    for (int r = 0; r < 4; r++)
      #pragma unroll
      for (int q = 0; q < 4; q++) {
        const SampleDistance o = {nb[r][q], nb[r][q] - same[r][q], (long long) ld[r][q]};
        if (mine) mine[(4 * ty + r) * E + 4 * tx + q] = o;
        else sdist_emit (out, ns, a0 + 4 * ty + r, b0 + 4 * tx + q, mirror, o);
      }
  }
  else {
    int *const acc_nb = lds, *const acc_nd = lds + E * E;
    u64 *const acc_ld = (u64 *) (lds + 2 * E * E);
    for (int x = tid; x < E * E; x += 256) { acc_nb[x] = 0; acc_nd[x] = 0; acc_ld[x] = 0ull; }
    __syncthreads ();
    #pragma unroll
    for (int r = 0; r < 4; r++)
      #pragma unroll
      for (int q = 0; q < 4; q++) {
        const int x = (4 * ty + r) * E + 4 * tx + q;
        if (nb[r][q]) atomicAdd (acc_nb + x, nb[r][q]);
        if (nb[r][q] - same[r][q]) atomicAdd (acc_nd + x, nb[r][q] - same[r][q]);
        if (ld[r][q]) atomicAdd (acc_ld + x, ld[r][q]);
      }
    __syncthreads ();
    for (int x = tid; x < E * E; x += 256) {
      const SampleDistance o = {acc_nb[x], acc_nd[x], (long long) acc_ld[x]};
      if (mine) mine[x] = o;
      else sdist_emit (out, ns, a0 + x / E, b0 + x % E, mirror, o);
    }
  }
}

template <int E>                                        // the tile's edge in samples: 8, 16, 32 or 64
__global__ __launch_bounds__ (256)
void sample_distances_kernel (const int16_t *__restrict__ gt, const int *__restrict__ lens, long n_sites, int ns,
                              int n_tiles, long per_slice, SampleDistance *__restrict__ partial, SampleDistance *__restrict__ out, const int *__restrict__ err)
{
  constexpr int CH = SDIST_CELLS / E;                   // sites of a chunk
  constexpr int T = E / 4;                              // pair threads along an edge of the tile
  constexpr int Z = 256 / (T * T);                      // thread groups that share the sites of a chunk
  static_assert (T * T * Z == 256 && CH % Z == 0 && E * E * 16 <= (Z > 1 ? 4 * SDIST_CELLS * 4 : 1 << 30), "tile shape");
  __shared__ __attribute__ ((aligned (16))) int lds[4 * SDIST_CELLS];
  __shared__ int l_max[2];                              // the largest length staged in a chunk (1023 at least), by the chunk's parity
  if (*(volatile const int *) err != 0) return;
  int *const gA = lds, *const lA = lds + SDIST_CELLS, *const gB = lds + 2 * SDIST_CELLS, *const lB = lds + 3 * SDIST_CELLS;
  int ti, tj;
  sdist_tile_pair (blockIdx.x, n_tiles, ti, tj);
  const int a0 = ti * E, b0 = tj * E;
  const long s_begin = blockIdx.y * per_slice, s_end = min (n_sites, s_begin + per_slice);
  const int tid = threadIdx.x, tx = tid % T, ty = (tid / T) % T, z = tid / (T * T);   // tx: along b (consecutive lanes, consecutive columns of the output), ty: along a
  int nb[4][4], same[4][4];                             // sites with both called; with the same call in both (n_differ is their difference)
  u32 ld32[4][4];                                       // length differences since the last flush ...
  u64 ld[4][4];                                         // ... and before it
  #pragma unroll
  for (int r = 0; r < 4; r++)
    #pragma unroll
    for (int q = 0; q < 4; q++) { nb[r][q] = 0; same[r][q] = 0; ld32[r][q] = 0u; ld[r][q] = 0ull; }
  if (tid == 0) l_max[0] = 1023;
  __syncthreads ();
  int parity = 0;
  for (long c0 = s_begin; c0 < s_end; c0 += CH, parity ^= 1) {
    sdist_stage<E> (gt, lens, ns, a0, b0, c0, s_end, tid, gA, lA, gB, lB, l_max + parity);
    __syncthreads ();
    if (tid == 0) l_max[parity ^ 1] = 1023;             // (the next chunk's: last read before the barrier that ended the chunk before, raised again behind the one that ends this)
    // A site adds |La - Lb| <= max (La, Lb) <= the chunk's largest length to a pair: the 32-bit sums of floor ((2^32 - 1) / largest)
    // sites cannot overflow.  With lengths as tracts have them that is more than a chunk, and the flush is the one at its end.
    const int flush_every = (int) min (0xffffffffu / (u32) l_max[parity], (u32) CH);
    const int n_here = (int) min ((long) CH, s_end - c0);
    int since = 0;
    for (int i = z; i < n_here; i += Z) {
      const int4 ga = *(const int4 *) (gA + i * E + 4 * ty), la = *(const int4 *) (lA + i * E + 4 * ty);
      const int4 gb = *(const int4 *) (gB + i * E + 4 * tx), lb = *(const int4 *) (lB + i * E + 4 * tx);
      const int gav[4] = {ga.x, ga.y, ga.z, ga.w}, lav[4] = {la.x, la.y, la.z, la.w}, gbv[4] = {gb.x, gb.y, gb.z, gb.w}, lbv[4] = {lb.x, lb.y, lb.z, lb.w};
      u32 ca[4], cb[4];                                 // all ones where the cell is called (a missing one has the sign bit), once per cell
      #pragma unroll
      for (int r = 0; r < 4; r++) {
        ca[r] = ~(u32) (gav[r] >> 31); cb[r] = ~(u32) (gbv[r] >> 31);
        asm ("" : "+v" (ca[r])); asm ("" : "+v" (cb[r]));   // (words from here on: told that they are sign masks, the compiler turns every use below into a compare and a select)
      }
      #pragma unroll
      for (int r = 0; r < 4; r++)
        #pragma unroll
        for (int q = 0; q < 4; q++) {                   // (masks, no branch: the sixteen pairs stay one straight run of instructions)
          const u32 c = ca[r] & cb[q];                  // all ones where both are called
          nb[r][q] -= (int) c;
          same[r][q] += gav[r] == gbv[q] ? 1 : 0;       // (a missing cell equals nothing in the other tile)
          const u32 x = ((u32) lav[r] & c) | ((u32) lbv[q] & ~c);   // b's own length where the pair does not count: a difference of 0
          ld32[r][q] = __usad (x, (u32) lbv[q], ld32[r][q]);   // (lengths are 0 .. 2^31 - 1)
        }
      if (++since == flush_every) {
        since = 0;
        #pragma unroll
        for (int r = 0; r < 4; r++)
          #pragma unroll
          for (int q = 0; q < 4; q++) { ld[r][q] += ld32[r][q]; ld32[r][q] = 0u; }
      }
    }
    #pragma unroll
    for (int r = 0; r < 4; r++)
      #pragma unroll
      for (int q = 0; q < 4; q++) { ld[r][q] += ld32[r][q]; ld32[r][q] = 0u; }
    __syncthreads ();
  }
  // where the sites are split, the whole tile goes to this workgroup's place in scratch: [slice][tile pair][E * E]
  SampleDistance *const mine = partial ? partial + ((long) blockIdx.y * gridDim.x + blockIdx.x) * (E * E) : nullptr;
  sdist_store_tile<E> (nb, same, ld, lds, mine, out, ns, a0, b0, ti != tj, tid);   // (a diagonal tile holds both halves itself)
}

// the slices' tiles summed: R lanes per cell of a tile pair (a power of two up to 16), lane l takes slices l, l + R, ...; the
// lanes' sums meet in shuffles (integer sums: the order does not show).  blockIdx.y: the matrix (N14 has one; N19 one per
// replicate, each with its slices in `partial` and its place in `out`)
__global__ __launch_bounds__ (256)
void sample_distances_reduce_kernel (const SampleDistance *__restrict__ partial, int n_slices, int n_tiles, int E, int R, int ns, SampleDistance *__restrict__ out,
                                     const int *__restrict__ err)
{
  if (*(volatile const int *) err != 0) return;
  const long cells = (long) n_tiles * (n_tiles + 1) / 2 * (E * E);
  partial += blockIdx.y * (n_slices * cells); out += blockIdx.y * ((long) ns * ns);
  const long n_threads = (long) gridDim.x * blockDim.x;   // (a multiple of R: the lanes of a cell stay together)
  const int l = threadIdx.x & (R - 1);
  for (long t = blockIdx.x * (long) blockDim.x + threadIdx.x; t < cells * R; t += n_threads) {   // (cells * R is a multiple of 64: a wavefront leaves the loop as one)
    const long x = t / R;
    int n_both = 0, n_differ = 0;
    u64 length_diff = 0;
    for (int s = l; s < n_slices; s += R) {
      const SampleDistance q = partial[s * cells + x];
      n_both += q.n_both; n_differ += q.n_differ; length_diff += (u64) q.length_diff;
    }
    for (int o = R >> 1; o; o >>= 1) {
      n_both += __shfl_xor (n_both, o, R); n_differ += __shfl_xor (n_differ, o, R); length_diff += shfl_xor64 (length_diff, o, R);
    }
    if (l == 0) {
      const int w = (int) (x % (E * E));
      int ti, tj;
      sdist_tile_pair ((int) (x / (E * E)), n_tiles, ti, tj);
      const SampleDistance o = {n_both, n_differ, (long long) length_diff};
      sdist_emit (out, ns, ti * E + w / E, tj * E + w % E, ti != tj, o);
    }
  }
}

// The host path that N14's entry and N19's weighted one share: where a helper takes a count of matrices or of batches, N14 passes 1.
// The argument checks behind an entry's own `null counter`, in their order: 0, or the code of the first that fails with its message set.
static int sdist_check_args (const char *fn, const tjamd_site *d_sites, long n_sites, const tjamd_allele *d_alleles, long n_alleles, const int16_t *d_genotype,
                             int n_samples, const tjamd_sample_distance *d_out)
{
  if (!d_out) return set_err (TJAMD_ERR_ARG, "%s: null d_out", fn);
  if (n_sites < 0 || n_alleles < 0) return set_err (TJAMD_ERR_ARG, "%s: n_sites %ld, n_alleles %ld: a count below 0", fn, n_sites, n_alleles);
  if ((n_sites > 0 && (!d_sites || !d_genotype)) || (n_alleles > 0 && !d_alleles)) return set_err (TJAMD_ERR_ARG, "%s: null site, allele or genotype buffer", fn);
  if (n_samples < 1 || n_samples > 4096) return set_err (TJAMD_ERR_ARG, "%s: n_samples %d outside 1..4096", fn, n_samples);
  if (n_alleles < n_sites) return set_err (TJAMD_ERR_ARG, "%s: %ld alleles for %ld sites (a site has at least one)", fn, n_alleles, n_sites);
  if (n_alleles >= (1l << 31)) return set_err (TJAMD_ERR_ARG, "%s: %ld alleles: 2^31 or more", fn, n_alleles);
  if (n_sites * (long) n_samples >= (1l << 31)) return set_err (TJAMD_ERR_ARG, "%s: %ld sites x %d samples: 2^31 cells or more", fn, n_sites, n_samples);
  return 0;
}

// The decomposition: tiles of E x E pairs on or above the diagonal, E = 64 where that (times the batches) alone gives half the
// workgroups aimed at (four per CU), otherwise 32, and 16 or 8 where the samples are no more; the sites in slices of whole chunks,
// as many as bring the workgroups to that number (few samples: many slices, their tiles summed from scratch; many samples: one,
// stored at once).  The scratch is one tile per workgroup: it is bounded by the workgroups aimed at, not by S^2 x slices (16 MB at
// most: 1024 tiles of edge 32); and the lengths of the check pass, an int per genotype cell: twice the matrix, 2 GB at 125 000
// sites x 4096 samples, under 8 GB at the 2^31 cells accepted.  They are ints because ref_length is one (runs of the test genomes
// pass 1500, the tests go to 2^31 - 1); an int16 copy for inputs whose lengths all fit would halve that and take a third off what a
// tile stages, behind a reduction over the sites ahead of the launch and four more instances of the tile kernel: not built.
struct SdistShape
{
  int E, n_tiles; long n_pairs, n_slices, per_slice;
  SdistShape (const tjamd_counter *c, long n_sites, int n_samples, long n_batches)
  {
    const long want = c->dist_blocks ? c->dist_blocks : 4l * c->n_cu, n_tiles64 = (n_samples + 63) / 64;
    E = n_samples <= 8 ? 8 : n_samples <= 16 ? 16 : n_tiles64 * (n_tiles64 + 1) / 2 * n_batches >= (want + 1) / 2 ? 64 : 32;
    n_tiles = (n_samples + E - 1) / E; n_pairs = (long) n_tiles * (n_tiles + 1) / 2;
    const long chunk = SDIST_CELLS / E, n_chunks = (n_sites + chunk - 1) / chunk;
    n_slices = std::max (1l, std::min (n_chunks, want / (n_pairs * n_batches)));
    per_slice = (n_chunks + n_slices - 1) / n_slices * chunk; n_slices = (n_sites + per_slice - 1) / per_slice;
  }
};
struct SdistScratch { int *err, *lens; SampleDistance *partial; };   // the error word; the lengths; the slices' tiles, or null where the sites are not split

template <class F> static void for_edge (int E, F &&f)
{ // E as a compile-time constant: f is called with std::integral_constant<int, E>, as with_width does for the record width
  if (E == 8) f (std::integral_constant<int, 8> ());
  else if (E == 16) f (std::integral_constant<int, 16> ());
  else if (E == 32) f (std::integral_constant<int, 32> ());
  else f (std::integral_constant<int, 64> ());
}

static long sdist_empty (tjamd_counter *c, const char *fn, tjamd_sample_distance *d_out, int n_samples, long n_matrices)
{ // no site: every pair of every matrix has nothing in common
  if (hipMemsetAsync (d_out, 0, (size_t) ((long) n_samples * n_samples * n_matrices) * sizeof (SampleDistance), c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: memset failed", fn);
  const int rc = read_back (c, fn, nullptr, nullptr, 0);
  return rc ? -rc : 0;
}

// the head of a call with sites: its scratch (a tile per workgroup and matrix where the sites are split), the stage's begin, the check pass
static int sdist_head (Stage &st, const char *fn, const SdistShape &s, const tjamd_site *d_sites, long n_sites, const tjamd_allele *d_alleles, long n_alleles,
                       const int16_t *d_genotype, int n_samples, long n_matrices, SdistScratch &x)
{
  tjamd_counter *const c = st.c; ScratchCut cut;
  cut.take (x.err, 64); cut.take (x.lens, (size_t) (n_sites * n_samples)); cut.take (x.partial, s.n_slices > 1 ? (size_t) (n_matrices * s.n_slices * s.n_pairs) * s.E * s.E : 0);
  if (const int rc = cut.commit (c)) return rc;
  if (s.n_slices == 1) x.partial = nullptr;
  if (hipMemsetAsync (x.err, 0, 256, c->stream) != hipSuccess) return set_err (TJAMD_ERR_HIP, "%s: memset failed", fn);
  const long check_items = std::max (n_sites * n_samples, n_alleles);
  st.begin ();
  hipLaunchKernelGGL (sample_distances_check_kernel, dim3 ((unsigned) std::min ((check_items + 255) / 256, 8l * c->n_cu)), dim3 (256), 0, c->stream,
                      (const Site *) d_sites, n_sites, (const Allele *) d_alleles, n_alleles, d_genotype, n_samples, x.lens, x.err);
  return 0;
}

// the error bits of sample_distances_check_kernel, in the order they are reported: 0 if none is up
static int sdist_refusal (const char *fn, u32 h_err, long n_alleles)
{
  for (const u32 bit : {16u, 8u, 32u}) if (h_err & bit) return site_bit_refused (fn, bit, n_alleles);
  if (h_err & 64u) return set_err (TJAMD_ERR_ARG, "%s: an allele's alt_length is outside 0..1023", fn);
  if (h_err & 128u) return set_err (TJAMD_ERR_ARG, "%s: a site's ref_length is below 0", fn);
  if (h_err & 1u) return set_err (TJAMD_ERR_ARG, "%s: a genotype cell is below -1 or above its site's n_alleles", fn);
  return 0;
}

// the tail, behind the tile kernels: the slices' tiles of every matrix summed into `out`, the stage's end, the error word (h_err: all its bits) and its shared bits decoded
static int sdist_tail (Stage &st, const char *fn, const SdistShape &s, const SdistScratch &x, int n_samples, long n_matrices, SampleDistance *out, long n_alleles, u32 &h_err)
{
  int R = 1;                                            // lanes per cell: as many as there are slices, 16 at most
  while (R < 16 && R < s.n_slices) R <<= 1;
  if (x.partial)
    hipLaunchKernelGGL (sample_distances_reduce_kernel, dim3 ((unsigned) std::min ((s.n_pairs * s.E * s.E * R + 255) / 256, 8l * st.c->n_cu), (unsigned) n_matrices), dim3 (256), 0,
                        st.c->stream, (const SampleDistance *) x.partial, (int) s.n_slices, s.n_tiles, s.E, R, n_samples, out, (const int *) x.err);
  st.end ();
  const int rc = read_back (st.c, fn, x.err, &h_err, 1);
  return rc ? rc : sdist_refusal (fn, h_err, n_alleles);
}

extern "C" long tjamd_sample_distances (tjamd_counter *c, const tjamd_site *d_sites, long n_sites, const tjamd_allele *d_alleles, long n_alleles,
                                        const int16_t *d_genotype, int n_samples, tjamd_sample_distance *d_out)
{
  static const char *fn = "tjamd_sample_distances";
  if (!c) return -set_err (TJAMD_ERR_ARG, "%s: null counter", fn);
  if (const int bad = sdist_check_args (fn, d_sites, n_sites, d_alleles, n_alleles, d_genotype, n_samples, d_out)) return -bad;
  Stage st (c, T_SAMPLE_DISTANCES);                     // (a refused call leaves no timing behind)
  if (const int bad = st.enter (fn, "the distances are summed")) return -bad;
  if (n_sites == 0) return sdist_empty (c, fn, d_out, n_samples, 1);
  const SdistShape s (c, n_sites, n_samples, 1);
  SdistScratch x; SampleDistance *const out = (SampleDistance *) d_out;
  if (const int bad = sdist_head (st, fn, s, d_sites, n_sites, d_alleles, n_alleles, d_genotype, n_samples, 1, x)) return -bad;
  for_edge (s.E, [&] (auto e) {
    hipLaunchKernelGGL (sample_distances_kernel<decltype (e)::value>, dim3 ((unsigned) s.n_pairs, (unsigned) s.n_slices), dim3 (256), 0, c->stream, d_genotype,
                        (const int *) x.lens, n_sites, n_samples, s.n_tiles, s.per_slice, x.partial, out, (const int *) x.err);
  });
  u32 h_err = 0;
  if (const int bad = sdist_tail (st, fn, s, x, n_samples, 1, out, n_alleles, h_err)) return -bad;
  st.done ();
  return n_sites;
}
TJ_LAST_MS (tjamd_last_sample_distances_ms, T_SAMPLE_DISTANCES)

// ---- N15: the single-linkage tree of the samples and its clusters at a threshold ---------------------------------------------
// N14's sample x sample matrix reduced to the minimum spanning forest of its pairs under the total order (key, a, b), and a list
// of links cut at a threshold into dense cluster ids; the rule as built is in include/tatajuba_linkage.h.  Boruvka and not Prim:
// a few passes over the matrix at memory rate, not n_samples dependent steps.
//   1. linkage_keys_kernel: tiles of 32 x 32 cells; a workgroup reads its tile (a, b) in rows and stages the tile (b, a), read in
//      rows as well, in LDS, so that a cell meets its mirror without a load that strides by a row.  Every cell is checked, and
//      a u64 key per cell goes to scratch (all ones: no edge, the diagonal, the padding column that makes a row's length even),
//      so that the rounds read 8 bytes a cell and not 16.  Raises the error flag; writes nothing of the caller's.
//   2. ceil (log2 n_samples) rounds of two kernels, launched without a look at the device in between:
//      (a) linkage_rowmin_kernel: a wavefront per row a takes the minimum of (key, b) over the b in another component, two keys
//          (16 bytes) a lane and load, then six cross-lane steps.  For one a, (min (a, b), max (a, b)) ascends with b: (key, b)
//          is the order of the rule.
//      (b, c) linkage_merge_kernel, one workgroup with the labels in LDS: the components' minima in two phases of LDS atomics
//          (the smallest key of a component, then the smallest packed pair among the rows that hold that key: integer minima, no
//          order shows); every component hooks onto the other end of its edge, a mutual pick is broken by the smaller label,
//          each chosen edge is appended once; the labels are flattened by pointer jumping.  A round with no edge at all sets
//          the `done` word, and every later kernel of the rounds returns at once when it reads it.  Nothing waits for another
//          workgroup.
//   3. linkage_sort_kernel: one workgroup sorts the links by (key, a, b) in LDS (a bitonic network over 12-byte entries: the
//      order needs 88 bits, the shared key-value sort has 64) and stores them.
// Up to 64 samples linkage_small_kernel does the three steps as one workgroup in one launch, the key matrix in LDS.
// linkage_clusters_kernel: one workgroup, labels in LDS; checks every link, hooks the larger label of a link at or under the
// threshold onto the smaller by an LDS atomic minimum, jumps pointers, until a pass changes nothing; a scan over the roots gives
// the dense ids.  DESIGN.md section 3.5, N15.

struct Link { int a, b; long long key; };
static_assert (sizeof (Link) == 16 && sizeof (Link) == sizeof (tjamd_link), "link layout");
struct LinkRowBest { u64 key; int b, pad; };            // a row's smallest (key, b) into another component; key LINK_NONE: none
struct LinkEdge { u64 key; u32 pair, pad; };            // a chosen edge before the sort: pair = a << 12 | b, a < b < 4096

#define LINK_NONE (~0ull)
#define LINK_TILE 32                                    // cells along an edge of a tile of the key pass
#define LINK_MAX 4096                                   // samples: the labels of one workgroup's LDS
// flags of a call: [0] error bits (1 a cell's values, 2 a cell and its mirror; clusters: 1 a link), [1] done (clusters: the number of clusters),
// [2] links appended so far, [3] rounds that merged something
static const char CELL_REFUSED[] = "%s: a cell has n_both < 0, n_differ < 0, n_differ > n_both or length_diff < 0";   // error bit 1
static const char MIRROR_REFUSED[] = "%s: a cell (a, b) differs from the cell (b, a)";                                   // error bit 2

// the early return of every kernel of the rounds: the call's error bits or its `done` word are up
__device__ __forceinline__ bool link_rounds_over (const int *flags) { return (((volatile const int *) flags)[0] | ((volatile const int *) flags)[1]) != 0; }

// the smallest (key, b) over the lanes of a wavefront, left in every lane: six cross-lane steps
__device__ __forceinline__ void wave_min_key_b (u64 &bk, int &bb)
{
  for (int o = 32; o; o >>= 1) {
    const u64 ok = shfl_xor64 (bk, o);
    const int ob = __shfl_xor (bb, o);
    if (ok < bk || (ok == bk && ob < bb)) { bk = ok; bb = ob; }
  }
}

// P places of LDS (a power of two) put into ascending order of (key, tie) by a workgroup of THREADS: the bitonic network, a
// compare-exchange a thread and step where P / 2 reaches that far.  The caller's barrier stands before the call; one stands
// behind every step.  Places to be left last hold all ones in both words.
template <int THREADS, class T>
__device__ __forceinline__ void lds_bitonic_sort (u64 *key, T *tie, int P)
{
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < P / 2; t += THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const u64 ki = key[i], kl = key[l];
        const T xi = tie[i], xl = tie[l];
        const bool above = ki > kl || (ki == kl && xi > xl);
        if (above == ((i & k) == 0)) { key[i] = kl; key[l] = ki; tie[i] = xl; tie[l] = xi; }
      }
      __syncthreads ();
    }
}

// the checks of a cell d against the rule and against its mirror m (error bits into `bad`), and its key: LINK_NONE for no edge
__device__ __forceinline__ u64 linkage_key (const SampleDistance &d, const SampleDistance &m, bool diagonal, int metric, int min_both, int &bad)
{
  if (d.n_both < 0 || d.n_differ < 0 || d.n_differ > d.n_both || d.length_diff < 0) { bad |= 1; return LINK_NONE; }
  if (d.n_both != m.n_both || d.n_differ != m.n_differ || d.length_diff != m.length_diff) { bad |= 2; return LINK_NONE; }
  if (diagonal || d.n_both < min_both) return LINK_NONE;
  // (min_both >= 1: the divisor is not 0; n_differ <= n_both < 2^31: the product is below 2^63 and the quotient 2^32 at most)
  return metric == TJAMD_LINK_DIFFER ? (u64) d.n_differ : metric == TJAMD_LINK_LENGTH ? (u64) d.length_diff : ((u64) d.n_differ << 32) / (u64) d.n_both;
}

// The tile (blockIdx.y, blockIdx.x) of one matrix: the kernels of N15 and N20 (a replicate per blockIdx.z) hand it their
// matrix.  -> the error bits of the tile's cells.  STORE: the keys go to scratch; without it the tile is checked and nothing is
// written.  key_max: a key at or above it raises bit 4 (N18's bound under AVERAGE; LINK_NONE: no bound)
template <bool STORE>
__device__ __forceinline__ int linkage_keys_tile (const SampleDistance *__restrict__ dist, int ns, int ld, int metric, int min_both, u64 key_max, u64 *__restrict__ keys)
{
  __shared__ __attribute__ ((aligned (16))) SampleDistance mirror[LINK_TILE * (LINK_TILE + 1)];   // (rows of 33: a column is read without bank conflicts)
  const int tid = threadIdx.x, a0 = blockIdx.y * LINK_TILE, b0 = blockIdx.x * LINK_TILE;
  #pragma unroll
  for (int j = 0; j < LINK_TILE * LINK_TILE / 256; j++) {   // the tile (b, a), in its rows
    const int x = tid + 256 * j, q = x / LINK_TILE, r = x % LINK_TILE, b = b0 + q, a = a0 + r;
    if (a < ns && b < ns) mirror[q * (LINK_TILE + 1) + r] = dist[(long) b * ns + a];
  }
  __syncthreads ();
  int bad = 0;
  #pragma unroll
  for (int j = 0; j < LINK_TILE * LINK_TILE / 256; j++) {
    const int x = tid + 256 * j, r = x / LINK_TILE, q = x % LINK_TILE, a = a0 + r, b = b0 + q;
    if (a >= ns || b >= ld) continue;
    u64 key = LINK_NONE;
    if (b < ns) key = linkage_key (dist[(long) a * ns + b], mirror[q * (LINK_TILE + 1) + r], a == b, metric, min_both, bad);
    if (key != LINK_NONE && key >= key_max) bad |= 4;
    if (STORE) keys[(long) a * ld + b] = key;           // (scratch)
  }
  return bad;
}

__global__ __launch_bounds__ (256)
void linkage_keys_kernel (const SampleDistance *__restrict__ dist, int ns, int ld, int metric, int min_both, u64 *__restrict__ keys, int *__restrict__ comp,
                          int *__restrict__ flags)
{
  const int tid = threadIdx.x, b0 = blockIdx.x * LINK_TILE;
  if (blockIdx.y == 0 && tid < LINK_TILE && b0 + tid < ld) comp[b0 + tid] = b0 + tid;   // every sample its own component (ld <= the array's length)
  const int bad = linkage_keys_tile<true> (dist, ns, ld, metric, min_both, LINK_NONE, keys);
  if (bad) atomicOr (flags, bad);
}

__device__ __forceinline__ void linkage_rowmin_body (const u64 *__restrict__ keys, int ns, int ld, const int *__restrict__ comp, LinkRowBest *__restrict__ rowbest, const int *__restrict__ flags)
{
  if (link_rounds_over (flags)) return;
  const int lane = threadIdx.x & 63, a = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (a >= ns) return;                                  // (a whole wavefront)
  const int ca = comp[a];
  const ulonglong2 *row = (const ulonglong2 *) (keys + (long) a * ld);   // (ld is even and the matrix starts on a 256-byte boundary: 16-byte loads)
  const int2 *comp2 = (const int2 *) comp;
  u64 bk = LINK_NONE;
  int bb = 0x7fffffff;
  #pragma unroll 4
  for (int p = lane; p < ld / 2; p += 64) {             // (a lane's b ascend: the first of equal keys stays)
    const ulonglong2 k = row[p];
    const int2 cb = comp2[p];
    if (cb.x != ca && k.x < bk) { bk = k.x; bb = 2 * p; }
    if (cb.y != ca && k.y < bk) { bk = k.y; bb = 2 * p + 1; }
  }
  wave_min_key_b (bk, bb);
  if (lane == 0) rowbest[a] = LinkRowBest {bk, bb, 0};
}
__global__ __launch_bounds__ (256)
void linkage_rowmin_kernel (const u64 *__restrict__ keys, int ns, int ld, const int *__restrict__ comp, LinkRowBest *__restrict__ rowbest, const int *__restrict__ flags)
{ linkage_rowmin_body (keys, ns, ld, comp, rowbest, flags); }

__device__ __forceinline__ void linkage_merge_body (const LinkRowBest *__restrict__ rowbest, int ns, int n_jump, int *__restrict__ comp, LinkEdge *__restrict__ edges, int *__restrict__ flags)
{
  __shared__ u64 cbkey[LINK_MAX];                       // per root: its component's smallest key ...
  __shared__ u32 cbpair[LINK_MAX];                      // ... and the smallest pair among the rows that hold it
  __shared__ unsigned short par[LINK_MAX];              // the labels while they are hooked and flattened
  __shared__ int n_new;
  if (link_rounds_over (flags)) return;
  const int tid = threadIdx.x, base = flags[2];
  u64 key[LINK_MAX / 1024];
  int other[LINK_MAX / 1024], cv[LINK_MAX / 1024];
  #pragma unroll
  for (int j = 0; j < LINK_MAX / 1024; j++) {
    const int v = tid + 1024 * j;
    key[j] = LINK_NONE; other[j] = 0; cv[j] = 0;
    if (v < ns) {
      const LinkRowBest rb = rowbest[v];
      key[j] = rb.key; other[j] = rb.b; cv[j] = comp[v];
      cbkey[v] = LINK_NONE; cbpair[v] = ~0u; par[v] = (unsigned short) cv[j];
    }
  }
  if (tid == 0) n_new = 0;
  __syncthreads ();
  #pragma unroll
  for (int j = 0; j < LINK_MAX / 1024; j++)
    if (key[j] != LINK_NONE) atomicMin (&cbkey[cv[j]], key[j]);
  __syncthreads ();
  #pragma unroll
  for (int j = 0; j < LINK_MAX / 1024; j++) {
    const int v = tid + 1024 * j;
    if (key[j] != LINK_NONE && key[j] == cbkey[cv[j]]) atomicMin (&cbpair[cv[j]], (u32) min (v, other[j]) << 12 | (u32) max (v, other[j]));
  }
  __syncthreads ();
  #pragma unroll
  for (int j = 0; j < LINK_MAX / 1024; j++) {
    const int v = tid + 1024 * j;
    if (v < ns && cv[j] == v && cbkey[v] != LINK_NONE) {   // a root with an edge: one end of it is in v's component, t is the other end's
      const u32 pair = cbpair[v];
      const int lo = (int) (pair >> 12), hi = (int) (pair & 4095u), t = comp[comp[lo] == v ? hi : lo];
      const bool mutual = cbpair[t] == pair && cbkey[t] == cbkey[v];   // (t chose the same edge: the one cycle a strict order allows)
      if (!mutual || v > t) {
        par[v] = (unsigned short) t;
        edges[base + atomicAdd (&n_new, 1)] = LinkEdge {cbkey[v], pair, 0u};   // (a forest: fewer than ns edges in all)
      }
    }
  }
  __syncthreads ();
  if (n_new == 0) { if (tid == 0) flags[1] = 1; return; }   // no component has an edge: the forest is complete
  for (int it = 0; it < n_jump; it++) {                 // a label read while its owner replaces it is an ancestor either way
    #pragma unroll
    for (int j = 0; j < LINK_MAX / 1024; j++) {
      const int v = tid + 1024 * j;
      if (v < ns) par[v] = par[par[v]];
    }
    __syncthreads ();
  }
  #pragma unroll
  for (int j = 0; j < LINK_MAX / 1024; j++) {
    const int v = tid + 1024 * j;
    if (v < ns) comp[v] = par[v];
  }
  if (tid == 0) { flags[2] = base + n_new; flags[3] += 1; }
}
__global__ __launch_bounds__ (1024)
void linkage_merge_kernel (const LinkRowBest *__restrict__ rowbest, int ns, int n_jump, int *__restrict__ comp, LinkEdge *__restrict__ edges, int *__restrict__ flags)
{ linkage_merge_body (rowbest, ns, n_jump, comp, edges, flags); }

__device__ __forceinline__ void linkage_sort_body (const LinkEdge *__restrict__ edges, int P, Link *__restrict__ out, const int *__restrict__ flags)
{
  __shared__ u64 skey[LINK_MAX];
  __shared__ u32 spair[LINK_MAX];
  if (((volatile const int *) flags)[0] != 0) return;
  const int tid = threadIdx.x, n = flags[2];            // (n <= P, a power of two up to LINK_MAX)
  for (int i = tid; i < P; i += 1024) {
    const bool in = i < n;
    skey[i] = in ? edges[i].key : LINK_NONE; spair[i] = in ? edges[i].pair : ~0u;
  }
  __syncthreads ();
  lds_bitonic_sort<1024> (skey, spair, P);
  for (int i = tid; i < n; i += 1024) out[i] = Link {(int) (spair[i] >> 12), (int) (spair[i] & 4095u), (long long) skey[i]};
}
__global__ __launch_bounds__ (1024)
void linkage_sort_kernel (const LinkEdge *__restrict__ edges, int P, Link *__restrict__ out, const int *__restrict__ flags)
{ linkage_sort_body (edges, P, out, flags); }

// Up to LINK_SMALL samples the key matrix fits in LDS (32 KB) and one workgroup does steps 1 to 3 in one launch: the same
// checks, rounds and sort, a lane per sample.  Waves take the rows in turn for the row minimum; thread v is sample v in the
// merge.  Barriers of one workgroup, nothing else, order the steps.
#define LINK_SMALL 64

// The body of the workgroup, for N15's kernel and N20's (a workgroup per replicate, the tree behind the links): -> the number
// of links, thread i < that number holding link i in `mine`; or -1 with the error bits in `bad_bits`, in every thread alike
__device__ __forceinline__ int linkage_small_body (const SampleDistance *__restrict__ dist, int ns, int metric, int min_both, int n_rounds, Link &mine, int &bad_bits)
{
  __shared__ u64 keys[LINK_SMALL * LINK_SMALL], rowkey[LINK_SMALL], cbkey[LINK_SMALL], ekey[LINK_SMALL];
  __shared__ u32 cbpair[LINK_SMALL], epair[LINK_SMALL];
  __shared__ int comp[LINK_SMALL], par[LINK_SMALL], rowb[LINK_SMALL], n_new, n_links, bad_any;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, v = tid;
  if (tid == 0) { n_links = 0; bad_any = 0; }
  if (tid < LINK_SMALL) { comp[tid] = tid; ekey[tid] = LINK_NONE; epair[tid] = ~0u; }
  __syncthreads ();
  int bad = 0;
  for (int x = tid; x < ns * ns; x += 256) {            // step 1: every cell beside its mirror (a matrix of 64 KB at most: the strided read is of no account)
    const int a = x / ns, b = x % ns;
    keys[a * LINK_SMALL + b] = linkage_key (dist[x], dist[b * ns + a], a == b, metric, min_both, bad);
  }
  if (bad) atomicOr (&bad_any, bad);
  __syncthreads ();
  bad_bits = bad_any;
  if (bad_any) return -1;                               // (the whole workgroup)
  for (int r = 0; r < n_rounds; r++) {                  // step 2
    for (int a = wave; a < ns; a += 4) {                // (a) a wavefront per row, lane b
      u64 bk = LINK_NONE;
      int bb = lane;
      if (lane < ns && comp[lane] != comp[a]) bk = keys[a * LINK_SMALL + lane];
      wave_min_key_b (bk, bb);
      if (lane == 0) { rowkey[a] = bk; rowb[a] = bb; cbkey[a] = LINK_NONE; cbpair[a] = ~0u; par[a] = comp[a]; }
    }
    if (tid == 0) n_new = 0;
    __syncthreads ();
    const bool has = v < ns && rowkey[v] != LINK_NONE;  // (b) the components' minima, in two phases
    const int cv = v < ns ? comp[v] : 0;
    if (has) atomicMin (&cbkey[cv], rowkey[v]);
    __syncthreads ();
    if (has && rowkey[v] == cbkey[cv]) atomicMin (&cbpair[cv], (u32) min (v, rowb[v]) << 12 | (u32) max (v, rowb[v]));
    __syncthreads ();
    if (v < ns && cv == v && cbkey[v] != LINK_NONE) {   // (c) hook and append, as linkage_merge_kernel does
      const u32 pair = cbpair[v];
      const int lo = (int) (pair >> 12), hi = (int) (pair & 4095u), t = comp[comp[lo] == v ? hi : lo];
      const bool mutual = cbpair[t] == pair && cbkey[t] == cbkey[v];
      if (!mutual || v > t) {
        par[v] = t;
        const int at = n_links + atomicAdd (&n_new, 1);
        ekey[at] = cbkey[v]; epair[at] = pair;
      }
    }
    __syncthreads ();
    if (n_new == 0) break;                              // (the whole workgroup) the forest is complete
    for (int it = 0; it < n_rounds; it++) {
      if (v < ns) par[v] = par[par[v]];
      __syncthreads ();
    }
    if (v < ns) comp[v] = par[v];
    if (tid == 0) n_links += n_new;
    __syncthreads ();
  }
  lds_bitonic_sort<256> (ekey, epair, LINK_SMALL);      // step 3: all 64 places, the empty ones last
  if (tid < n_links) mine = Link {(int) (epair[tid] >> 12), (int) (epair[tid] & 4095u), (long long) ekey[tid]};
  return n_links;
}

__global__ __launch_bounds__ (256)
void linkage_small_kernel (const SampleDistance *__restrict__ dist, int ns, int metric, int min_both, int n_rounds, Link *__restrict__ out, int *__restrict__ flags)
{
  const int tid = threadIdx.x;
  Link mine;
  int bad;
  const int n_links = linkage_small_body (dist, ns, metric, min_both, n_rounds, mine, bad);
  if (n_links < 0) { if (tid == 0) flags[0] = bad; return; }   // (the whole workgroup; nothing of the caller's is written)
  if (tid < n_links) out[tid] = mine;
  if (tid == 0) flags[2] = n_links;
}

// the argument checks that tjamd_sample_linkage and tjamd_sample_agglomerate share, in their order: 0, or the code of the first
// that fails with its message set
static int link_check_args (const char *fn, tjamd_counter *c, const tjamd_sample_distance *d_dist, int n_samples, int metric, int min_both, const tjamd_link *d_links)
{
  if (!c) return set_err (TJAMD_ERR_ARG, "%s: null counter", fn);
  if (!d_dist) return set_err (TJAMD_ERR_ARG, "%s: null d_dist", fn);
  if (!d_links && n_samples > 1) return set_err (TJAMD_ERR_ARG, "%s: null d_links", fn);
  if (n_samples < 1 || n_samples > LINK_MAX) return set_err (TJAMD_ERR_ARG, "%s: n_samples %d outside 1..4096", fn, n_samples);
  if (metric < TJAMD_LINK_DIFFER || metric > TJAMD_LINK_DIFFER_RATE) return set_err (TJAMD_ERR_ARG, "%s: metric %d outside 0..2", fn, metric);
  if (min_both < 1) return set_err (TJAMD_ERR_ARG, "%s: min_both %d below 1", fn, min_both);
  return 0;
}

// The shape of a call on n_samples > 1 samples.  ld: a row of the key matrix, an even number of cells for 16-byte loads; P: the
// places of the sort, a power of two that holds n_samples - 1 links
struct LinkShape
{
  int ld, P;
  explicit LinkShape (int n_samples) : ld ((n_samples + 1) & ~1), P (2) { while (P < n_samples - 1) P <<= 1; }
};

// step 1 of both entries: the key pass, a workgroup per tile
static void launch_linkage_keys (tjamd_counter *c, const tjamd_sample_distance *d_dist, int n_samples, int ld, int metric, int min_both, u64 *keys, int *comp, int *flags)
{
  hipLaunchKernelGGL (linkage_keys_kernel, dim3 ((unsigned) ((ld + LINK_TILE - 1) / LINK_TILE), (unsigned) ((n_samples + LINK_TILE - 1) / LINK_TILE)), dim3 (256), 0, c->stream,
                      (const SampleDistance *) d_dist, n_samples, ld, metric, min_both, keys, comp, flags);
}

extern "C" long tjamd_sample_linkage (tjamd_counter *c, const tjamd_sample_distance *d_dist, int n_samples, int metric, int min_both, tjamd_link *d_links)
{
  static const char *fn = "tjamd_sample_linkage";
  int rc = link_check_args (fn, c, d_dist, n_samples, metric, min_both, d_links);
  if (rc) return -rc;
  Stage st (c, T_SAMPLE_LINKAGE);                       // (a refused call leaves no timing behind)
  if (const int bad = st.enter (fn, "the tree is built")) return -bad;
  if (n_samples == 1) {                                 // one sample: no pair, no kernel
    rc = read_back (c, fn, nullptr, nullptr, 0);
    return rc ? -rc : 0;
  }
  const LinkShape shape (n_samples);
  const int ld = shape.ld, P = shape.P;
  int n_rounds = 0;
  while ((1 << n_rounds) < n_samples) n_rounds++;       // every round at least halves the components that still have an edge
  const bool small = n_samples <= LINK_SMALL && c->link_small;   // one workgroup, one launch
  ScratchCut cut;
  int *flags, *comp; LinkRowBest *rowbest; LinkEdge *edges; u64 *keys;
  cut.take (comp, small ? 0 : (size_t) ld + 64); cut.take (rowbest, small ? 0 : (size_t) n_samples); cut.take (edges, small ? 0 : (size_t) n_samples);
  cut.take (keys, small ? 0 : (size_t) n_samples * ld);
  rc = commit_with_flags (cut, c, fn, flags);
  if (rc) return -rc;
  st.begin ();
  if (small)
    hipLaunchKernelGGL (linkage_small_kernel, dim3 (1), dim3 (256), 0, c->stream, (const SampleDistance *) d_dist, n_samples, metric, min_both, n_rounds, (Link *) d_links, flags);
  else {
    launch_linkage_keys (c, d_dist, n_samples, ld, metric, min_both, keys, comp, flags);
    for (int r = 0; r < n_rounds; r++) {
      hipLaunchKernelGGL (linkage_rowmin_kernel, dim3 ((unsigned) ((n_samples + 3) / 4)), dim3 (256), 0, c->stream, (const u64 *) keys, n_samples, ld, (const int *) comp,
                          rowbest, (const int *) flags);
      hipLaunchKernelGGL (linkage_merge_kernel, dim3 (1), dim3 (1024), 0, c->stream, (const LinkRowBest *) rowbest, n_samples, n_rounds, comp, edges, flags);
    }
    hipLaunchKernelGGL (linkage_sort_kernel, dim3 (1), dim3 (1024), 0, c->stream, (const LinkEdge *) edges, P, (Link *) d_links, (const int *) flags);
  }
  st.end ();
  u32 h_flags[4] = {0, 0, 0, 0};
  rc = read_back (c, fn, flags, h_flags, 4);
  if (rc) return -rc;
  if (h_flags[0] & 1u) return -set_err (TJAMD_ERR_ARG, CELL_REFUSED, fn);
  if (h_flags[0] & 2u) return -set_err (TJAMD_ERR_ARG, MIRROR_REFUSED, fn);
  st.done ();
  return (long) h_flags[2];
}
TJ_LAST_MS (tjamd_last_sample_linkage_ms, T_SAMPLE_LINKAGE)

__global__ __launch_bounds__ (1024)
void linkage_clusters_kernel (const Link *__restrict__ links, long n_links, int ns, long long threshold, int *__restrict__ cluster, int *__restrict__ flags)
{
  __shared__ int lab[LINK_MAX], rank[LINK_MAX], wsum[16];
  volatile int *const vlab = lab;                       // (labels move under the reader: every read is a load)
  const int tid = threadIdx.x;
  int bad = 0;
  for (long i = tid; i < n_links; i += 1024) {          // every link, whatever the threshold, before anything is written
    const Link l = links[i];
    if (l.a < 0 || l.a >= l.b || l.b >= ns || l.key < 0) bad = 1;
  }
  if (__syncthreads_or (bad)) { if (tid == 0) flags[0] = 1; return; }
  for (int v = tid; v < ns; v += 1024) lab[v] = v;
  __syncthreads ();
  // lab[v] <= v and lab[v] is in v's component, always.  A pass that changes nothing: the two ends of every link have one label,
  // so a component has one label, a member of it that is at most its smallest member.
  while (threshold >= 0) {
    int changed = 0;
    for (long i = tid; i < n_links; i += 1024) {
      const Link l = links[i];
      if (l.key > threshold) continue;
      const int la = vlab[l.a], lb = vlab[l.b];
      if (la != lb) { atomicMin (&lab[max (la, lb)], min (la, lb)); changed = 1; }
    }
    if (!__syncthreads_or (changed)) break;
    for (;;) {                                          // pointer jumping until every label is a root
      int jumped = 0;
      for (int v = tid; v < ns; v += 1024) {
        const int p = vlab[v], pp = vlab[p];
        if (pp != p) { vlab[v] = pp; jumped = 1; }
      }
      if (!__syncthreads_or (jumped)) break;
    }
  }
  // dense ids: the roots counted in the order of their index, four consecutive samples a thread
  int mine = 0;
  #pragma unroll
  for (int j = 0; j < LINK_MAX / 1024; j++) {
    const int v = (LINK_MAX / 1024) * tid + j;
    if (v < ns && lab[v] == v) mine++;
  }
  int n_clusters;
  int at = block_exclusive_scan_1024 (mine, tid, wsum, n_clusters);
  #pragma unroll
  for (int j = 0; j < LINK_MAX / 1024; j++) {
    const int v = (LINK_MAX / 1024) * tid + j;
    if (v < ns && lab[v] == v) rank[v] = at++;
  }
  __syncthreads ();
  for (int v = tid; v < ns; v += 1024) cluster[v] = rank[lab[v]];
  if (tid == 0) flags[1] = n_clusters;
}

extern "C" long tjamd_linkage_clusters (tjamd_counter *c, const tjamd_link *d_links, long n_links, int n_samples, long long threshold, int *d_cluster)
{
  static const char *fn = "tjamd_linkage_clusters";
  if (!c) return -set_err (TJAMD_ERR_ARG, "%s: null counter", fn);
  if (!d_cluster) return -set_err (TJAMD_ERR_ARG, "%s: null d_cluster", fn);
  if (n_links < 0 || n_links > (1l << 24)) return -set_err (TJAMD_ERR_ARG, "%s: n_links %ld outside 0..2^24", fn, n_links);
  if (!d_links && n_links > 0) return -set_err (TJAMD_ERR_ARG, "%s: null d_links", fn);
  if (n_samples < 1 || n_samples > LINK_MAX) return -set_err (TJAMD_ERR_ARG, "%s: n_samples %d outside 1..4096", fn, n_samples);
  Stage st (c, T_LINKAGE_CLUSTERS);                     // (a refused call leaves no timing behind)
  if (const int bad = st.enter (fn, "the tree is cut")) return -bad;
  ScratchCut cut;
  int *flags;
  int rc = commit_with_flags (cut, c, fn, flags);
  if (rc) return -rc;
  st.begin ();
  hipLaunchKernelGGL (linkage_clusters_kernel, dim3 (1), dim3 (1024), 0, c->stream, (const Link *) d_links, n_links, n_samples, threshold, d_cluster, flags);
  st.end ();
  u32 h_flags[2] = {0, 0};
  rc = read_back (c, fn, flags, h_flags, 2);
  if (rc) return -rc;
  if (h_flags[0]) return -set_err (TJAMD_ERR_ARG, "%s: a link has a < 0, a >= b, b >= n_samples or key < 0", fn);
  st.done ();
  return (long) h_flags[1];
}
TJ_LAST_MS (tjamd_last_linkage_clusters_ms, T_LINKAGE_CLUSTERS)

// ---- N16: the sites that set a group of samples apart from the rest --------------------------------------------------------
// The site x sample genotype matrix reduced per site under the key (group, genotype); the rule as built is in
// include/tatajuba_groups.h.  Three steps: a pass that makes every check, counts the marks of every site into scratch and sums
// the marks of every group there, and writes nothing of the caller's; the shared scan of the sites' counts; a pass that returns
// while the error flag is up and otherwise computes every site again (the matrix is 2 bytes a cell; the calls are not kept) and
// writes the four outputs, a mark at its site's offset plus its rank among the site's marks.  The two passes are one kernel
// compiled twice.  A site's work has two forms, chosen by n_samples alone:
//   up to 64 samples, group_sites_small_kernel: a wavefront per site, a lane per sample.  The membership masks do not depend on
//     the site: lane r keeps the r-th smallest group that has a member and __ballot (label == group), made once per wavefront.
//     Per site called = __ballot (g >= 0) among those who take part; per group with a member the genotype x of its first called
//     lane and same = __ballot (g == x): fixed iff the group's called mask lies inside `same`, n_outside the popcount of `same`
//     among the other groups' called.  All of it is wave-uniform 64-bit mask arithmetic; no LDS atomic.
//   beyond, group_sites_large_kernel: a workgroup of 1024 walks a run of sites, a thread keeping the labels of its four
//     samples in registers.  Per site LDS atomics into a table per group (count, smallest and largest genotype: fixed iff they
//     are equal) and a table of counts per genotype (0 .. n_alleles <= n_samples: hence that bound); a wavefront first folds its
//     lanes of equal (group, genotype), up to eight such keys, into one atomic each, because few groups and few alleles are the
//     usual case and would otherwise meet on one address.  Then a thread per group forms n_outside = count[fixed] - n_called and
//     the mark, and clears its own entry; the marks of 64 groups are a __ballot word in LDS, from which a site's count, its
//     first group and a mark's rank are popcounts.  The genotype counts are cleared up to the site's n_alleles.  66 KB of LDS: two
//     workgroups to a CU.  Nothing waits for another workgroup.
// Global atomics: the error flag, and a group's marks once per workgroup (from registers and LDS, not per site) into scratch,
// from where the second pass copies them out: d_group_marks is not touched by a refused call.  DESIGN.md section 3.5, N16.

struct GroupCall { int n_called, fixed, n_outside, mark; };
struct GroupSite { int n_called, n_genotypes, n_marks, first_group; };
struct GroupMark { int site, group, genotype, n_called; };
static_assert (sizeof (GroupCall) == 16 && sizeof (GroupCall) == sizeof (tjamd_group_call), "group call layout");
static_assert (sizeof (GroupSite) == 16 && sizeof (GroupSite) == sizeof (tjamd_group_site), "group site layout");
static_assert (sizeof (GroupMark) == 16 && sizeof (GroupMark) == sizeof (tjamd_group_mark), "group mark layout");

// The constants of the site marks, one set for the groups of N16 and the clades of N17 (a key: a group or a node of the tree)
#define CLD_MAX 4096                                    // samples, keys and, by the rule's bound, alleles of a site
#define CLD_SMALL 64                                    // samples up to which a wavefront takes a site
#define CLD_THREADS 1024
#define CLD_PER (CLD_MAX / CLD_THREADS)                 // samples or leaf positions, and keys, of a thread of the second form
#define CLD_FOLD 8                                      // distinct keys a wavefront folds into a lane each before its lanes go alone
#define CLD_WAVE_SITES 64                               // sites a workgroup of the first form is sized for, where there are that many
#define CLD_NONE 0x7fffffff
// words of a call: [0] error bits, [1] the number of marks (the scan's total); from word 64 on: the marks of every key.  The
// error bits of tjamd_group_sites: 1 a label, 2 a site's n_alleles, 4 a cell; of tjamd_clade_sites: 1 the order, 2 a node, 4 a
// site's n_alleles, 8 a cell
struct MarkArgs                                         // what the two entries share; GroupArgs and CladeArgs add their own
{
  int ns, n_keys, min_called; const Site *sites; long n_sites; const int16_t *geno;   // (the three counts first: with the sites first the second pass of both workgroup forms takes 72 registers and more)
  GroupCall *calls; GroupSite *site_out; int *key_marks; GroupMark *marks; long cap;
  int *flags, *km; u32 *cnt;                            // km: the marks of every key, in scratch; cnt: a site's marks (written by the first pass), then their offsets (read by the second)
};
struct GroupArgs : MarkArgs { const int *group; };

// The start of the second pass: false while the error flag is up, and the pass returns; workgroup 0 copies the marks of every
// key out of scratch.
template <int THREADS>
__device__ __forceinline__ bool marks_emit_begin (const MarkArgs &A)
{
  if (((volatile const int *) A.flags)[0] != 0) return false;
  if (A.key_marks && blockIdx.x == 0)
    for (int j = threadIdx.x; j < A.n_keys; j += THREADS) A.key_marks[j] = A.km[j];
  return true;
}

// The rule of a mark for a key with a fixed genotype: enough called members, no called sample outside them carries it, and
// somebody outside is called.
__device__ __forceinline__ int mark_rule (int n_called, int min_called, int n_outside, bool outside_called)
{
  return n_called >= min_called && n_outside == 0 && outside_called;
}

// The end of the first pass of a wavefront form: the error bits; lane r of every wavefront holds the marks of one key, the same
// key in all four wavefronts, and the first n lanes of the workgroup add theirs (key: that of this thread's lane) into scratch.
__device__ __forceinline__ void marks_count_end_small (const MarkArgs &A, int bad, int (*s_marks)[CLD_SMALL], int my_marks, int n, int key)
{
  const int tid = threadIdx.x;
  if (bad) atomicOr (A.flags, bad);
  s_marks[tid >> 6][tid & 63] = my_marks;
  __syncthreads ();
  if (tid < n) {
    const int sum = s_marks[0][tid] + s_marks[1][tid] + s_marks[2][tid] + s_marks[3][tid];
    if (sum) atomicAdd (&A.km[key], sum);
  }
}

// The end of the first pass of a workgroup form: the error bits, and the marks of this thread's keys (tid + CLD_THREADS * j).
__device__ __forceinline__ void marks_count_end (const MarkArgs &A, int bad, const int (&kmarks)[CLD_PER], int tid)
{
  if (bad) atomicOr (A.flags, bad);
  #pragma unroll
  for (int j = 0; j < CLD_PER; j++)
    if (kmarks[j]) atomicAdd (&A.km[tid + CLD_THREADS * j], kmarks[j]);
}

// A wavefront's active lanes folded by their keys before an LDS atomic: up to CLD_FOLD distinct keys elect a lane each, which
// calls add (the number of its lanes); the lanes that are left call add (1).  Few keys are the usual case and would otherwise
// meet on one address.
template <class Add>
__device__ __forceinline__ void fold_equal_keys (bool active, int key, int lane, Add add)
{
  u64 rem = __ballot (active);
  #pragma unroll 1
  for (int it = 0; it < CLD_FOLD && rem; it++) {
    const int j = __ffsll ((long long) rem) - 1;
    const u64 m = __ballot (active && key == __builtin_amdgcn_readlane (key, j));
    if (lane == j) add ((int) __popcll (m));
    rem &= ~m;
    if ((m >> lane) & 1ull) active = false;
  }
  if (active) add (1);
}

// The tail of a site in the workgroup forms, in four steps.  x_cnt: the carriers of every genotype 0 .. na; markbits: a word
// per 64 keys, bit set for a mark (the words of keys beyond n_keys stay 0).
// 1. before the barrier that ends the calls: the genotypes that somebody carries, added to *s_ngeno
__device__ __forceinline__ void site_count_genotypes (const int *x_cnt, int na, int tid, int *s_ngeno)
{
  int nz = 0;
  for (int x = tid; x <= na; x += CLD_THREADS) nz += x_cnt[x] != 0;
  for (int o = 32; o; o >>= 1) nz += __shfl_xor (nz, o);
  if (nz && (tid & 63) == 0) atomicAdd (s_ngeno, nz);
}
// 2. behind that barrier: the first wavefront turns the mark words into the site's count and first key; thread 0 writes the
//    count for the scan, or the site's record (called: the site's called samples; n_genotypes: step 1's sum), and then calls
//    clear (), which zeroes the form's LDS words of a site
template <bool EMIT, class Clear>
__device__ __forceinline__ void site_marks_total (const MarkArgs &A, long i, const u64 *markbits, int tid, int called, const int &n_genotypes, Clear clear)
{
  if (tid >= 64) return;
  const u64 w = markbits[tid];
  int n_marks = __popcll (w), first = w ? tid * 64 + __ffsll ((long long) w) - 1 : CLD_NONE;
  for (int o = 32; o; o >>= 1) { n_marks += __shfl_xor (n_marks, o); first = min (first, __shfl_xor (first, o)); }
  if (tid == 0) {
    if (!EMIT) A.cnt[i] = (u32) n_marks;
    else if (A.site_out) A.site_out[i] = GroupSite {called, n_genotypes, n_marks, first == CLD_NONE ? -1 : first};
    clear ();
  }
}
// 3. the place of key j's mark in the list: the site's offset, the marks in the words below its own, the bits below it there
__device__ __forceinline__ long site_mark_place (const MarkArgs &A, long i, const u64 *markbits, int j)
{
  long pos = (long) A.cnt[i] + __popcll (markbits[j >> 6] & ((1ull << (j & 63)) - 1ull));
  #pragma unroll 1
  for (int w = 0; w < (j >> 6); w++) pos += __popcll (markbits[w]);
  return pos;
}
// 4. before the barrier that ends the site: the carriers cleared, as far as this site could touch them
__device__ __forceinline__ void site_clear_genotypes (int *x_cnt, int na, int tid)
{
  for (int x = tid; x <= na; x += CLD_THREADS) x_cnt[x] = 0;
}

template <bool EMIT>
__global__ __launch_bounds__ (256)
void group_sites_small_kernel (const GroupArgs A)
{
  __shared__ int s_marks[4][CLD_SMALL];
  if (EMIT && !marks_emit_begin<256> (A)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ns = A.ns, n_groups = A.n_keys;
  int bad = 0, label = -1;
  if (lane < ns) {
    label = A.group[lane];
    if (label < -1 || label >= n_groups) { bad |= 1; label = -1; }
  }
  const u64 taking = __ballot (label >= 0);
  int gid = CLD_NONE, ng = 0, my_marks = 0;             // lane r: the r-th smallest group that has a member, and its members
  u64 gmask = 0;
  for (int cur = -1; ng < CLD_SMALL; ng++) {
    int next = label > cur ? label : CLD_NONE;
    for (int o = 32; o; o >>= 1) next = min (next, __shfl_xor (next, o));
    next = __builtin_amdgcn_readfirstlane (next);
    if (next == CLD_NONE) break;
    const u64 m = __ballot (label == next);
    if (lane == ng) { gid = next; gmask = m; }
    cur = next;
  }
  for (long i = (long) blockIdx.x * 4 + wave; i < A.n_sites; i += (long) gridDim.x * 4) {
    const int na = A.sites[i].n_alleles;
    if (na < 1 || na > ns) {                            // (the whole wavefront)
      bad |= 2;
      if (!EMIT && lane == 0) A.cnt[i] = 0;
      continue;
    }
    int g = -1;
    if (lane < ns) {
      g = A.geno[i * ns + lane];
      if (g < -1 || g > na) { bad |= 4; g = -1; }
    }
    const u64 called = __ballot (g >= 0) & taking;      // those who take part only: nobody else is a member or an outsider
    const long at = EMIT ? (long) A.cnt[i] : 0;
    int n_marks = 0, first = -1;
    GroupCall mine = {0, -1, 0, 0};                     // lane r: the call of the r-th group
    for (int r = 0; r < ng; r++) {
      const u64 members = readlane64 (gmask, r), cm = called & members, others = called & ~members;
      GroupCall q = {(int) __popcll (cm), -1, 0, 0};
      if (cm) {
        const int x = __builtin_amdgcn_readlane (g, __ffsll ((long long) cm) - 1);
        const u64 same = __ballot (g == x);
        q.fixed = (cm & ~same) ? -2 : x;
        if (q.fixed >= 0) {
          q.n_outside = __popcll (same & others);
          q.mark = mark_rule (q.n_called, A.min_called, q.n_outside, others != 0);
        }
      }
      if (q.mark) {
        const int G = __builtin_amdgcn_readlane (gid, r);
        if (first < 0) first = G;
        if (EMIT && A.marks && lane == 0 && at + n_marks < A.cap) A.marks[at + n_marks] = GroupMark {(int) i, G, q.fixed, q.n_called};
        n_marks++;
        if (!EMIT && lane == r) my_marks++;
      }
      if (EMIT && lane == r) mine = q;
    }
    if (!EMIT) {
      if (lane == 0) A.cnt[i] = (u32) n_marks;
      continue;
    }
    if (A.site_out) {
      int n_genotypes = 0;
      for (u64 rem = called; rem; n_genotypes++)        // one step per distinct genotype
        rem &= ~__ballot (g == __builtin_amdgcn_readlane (g, __ffsll ((long long) rem) - 1));
      if (lane == 0) A.site_out[i] = GroupSite {(int) __popcll (called), n_genotypes, n_marks, first};
    }
    if (A.calls)
      for (int base = 0; base < n_groups; base += 64) { // a lane per group: the place of G among the groups that have a member
        const int G = base + lane;
        int lo = 0, hi = ng;
        for (int it = 0; it < 7; it++) {
          const int mid = (lo + hi) >> 1, v = __shfl (gid, mid & 63);
          if (lo < hi) { if (v < G) lo = mid + 1; else hi = mid; }
        }
        const int r = lo & 63, at_r = __shfl (gid, r);  // (every lane takes part in every exchange: a lane that sits out is read as 0)
        const bool has = lo < ng && at_r == G;
        GroupCall q = {__shfl (mine.n_called, r), __shfl (mine.fixed, r), __shfl (mine.n_outside, r), __shfl (mine.mark, r)};
        if (!has) q = GroupCall {0, -1, 0, 0};
        if (G < n_groups) A.calls[i * n_groups + G] = q;
      }
  }
  if (!EMIT) marks_count_end_small (A, bad, s_marks, my_marks, ng, gid);   // every wavefront has the same list of groups
}

template <bool EMIT>
__global__ __launch_bounds__ (CLD_THREADS)
void group_sites_large_kernel (const GroupArgs A, long per_block)
{
  __shared__ int g_cnt[CLD_MAX], g_min[CLD_MAX], g_max[CLD_MAX], x_cnt[CLD_MAX + 1];
  __shared__ u64 markbits[CLD_MAX / 64];
  __shared__ int s_called, s_ngeno;
  if (EMIT && !marks_emit_begin<CLD_THREADS> (A)) return;
  const int tid = threadIdx.x, lane = tid & 63, ns = A.ns, n_groups = A.n_keys;
  int bad = 0, label[CLD_PER], gmarks[CLD_PER];
  #pragma unroll
  for (int j = 0; j < CLD_PER; j++) {
    const int s = tid + CLD_THREADS * j;
    label[j] = -1; gmarks[j] = 0;
    if (s < ns) {
      label[j] = A.group[s];
      if (label[j] < -1 || label[j] >= n_groups) { bad |= 1; label[j] = -1; }
    }
    g_cnt[s] = 0; g_min[s] = CLD_NONE; g_max[s] = -1; x_cnt[s] = 0;
  }
  if (tid < CLD_MAX / 64) markbits[tid] = 0;
  if (tid == 0) { x_cnt[CLD_MAX] = 0; s_called = 0; s_ngeno = 0; }
  __syncthreads ();
  const long i0 = (long) blockIdx.x * per_block, i1 = min (A.n_sites, i0 + per_block);
  for (long i = i0; i < i1; i++) {
    const int na = A.sites[i].n_alleles;
    if (na < 1 || na > ns) {                            // (the whole workgroup; the tables are clean)
      bad |= 2;
      if (!EMIT && tid == 0) A.cnt[i] = 0;
      continue;
    }
    #pragma unroll
    for (int j = 0; j < CLD_PER; j++) {
      const int s = tid + CLD_THREADS * j;
      if (CLD_THREADS * j + (tid & ~63) >= ns) break;   // (a whole wavefront)
      int g = -1;
      if (s < ns) {
        g = A.geno[i * ns + s];
        if (g < -1 || g > na) { bad |= 4; g = -1; }
      }
      const bool active = g >= 0 && label[j] >= 0;
      const int n = __popcll (__ballot (active));
      if (n && lane == 0) atomicAdd (&s_called, n);
      const int G = label[j];                           // the two tables of the site, lanes of one (group, genotype) folded (g <= 4096)
      fold_equal_keys (active, G << 13 | g, lane, [&] (int n) { atomicAdd (&g_cnt[G], n); atomicMin (&g_min[G], g); atomicMax (&g_max[G], g); atomicAdd (&x_cnt[g], n); });
    }
    __syncthreads ();
    const int all_called = s_called;
    u32 marked = 0;                                     // bit j: this thread's j-th group is marked here
    #pragma unroll
    for (int j = 0; j < CLD_PER; j++) {                 // a thread per group
      const int G = tid + CLD_THREADS * j;
      if (CLD_THREADS * j + (tid & ~63) >= n_groups) continue;   // (a whole wavefront)
      int nc = 0, fixed = -1, n_outside = 0, mark = 0;
      if (G < n_groups) {
        nc = g_cnt[G];
        if (nc) {
          const int lo = g_min[G], hi = g_max[G];
          fixed = lo == hi ? lo : -2;
          if (fixed >= 0) {
            n_outside = x_cnt[fixed] - nc;
            mark = mark_rule (nc, A.min_called, n_outside, all_called > nc);
          }
          if (!(EMIT && mark)) { g_cnt[G] = 0; g_min[G] = CLD_NONE; g_max[G] = -1; }   // (a marked group's entry is its record until the list has it)
        }
        if (EMIT && A.calls) A.calls[i * n_groups + G] = GroupCall {nc, fixed, n_outside, mark};
      }
      const u64 mb = __ballot (mark != 0);
      if (lane == 0) markbits[G >> 6] = mb;
      if (!EMIT) gmarks[j] += mark;
      marked |= (u32) mark << j;
    }
    if (EMIT && A.site_out) site_count_genotypes (x_cnt, na, tid, &s_ngeno);
    __syncthreads ();
    site_marks_total<EMIT> (A, i, markbits, tid, all_called, s_ngeno, [&] { s_called = 0; s_ngeno = 0; });
    if (EMIT && marked) {
      #pragma unroll 1
      for (int j = 0; j < CLD_PER; j++) {
        if (!((marked >> j) & 1u)) continue;
        const int G = tid + CLD_THREADS * j, nc = g_cnt[G], fixed = g_min[G];
        g_cnt[G] = 0; g_min[G] = CLD_NONE; g_max[G] = -1;
        if (!A.marks) continue;
        const long pos = site_mark_place (A, i, markbits, G);
        if (pos < A.cap) A.marks[pos] = GroupMark {(int) i, G, fixed, nc};
      }
    }
    site_clear_genotypes (x_cnt, na, tid);
    __syncthreads ();
  }
  if (!EMIT) marks_count_end (A, bad, gmarks, tid);
}

// The host side of the two entries.  An entry checks its arguments in this order: mark_check_head (), its own checks of its
// keys, mark_check_tail (); then mark_sites () runs the three steps.  Each check returns 0, or the code of the first rule that is
// broken with its message set.
struct MarkCall                                         // the arguments that both entries have, as the caller gave them
{
  const char *fn; tjamd_counter *c; const tjamd_site *d_sites; long n_sites; const int16_t *d_genotype; int n_samples, n_keys, min_called;
  tjamd_group_call *d_calls; tjamd_group_site *d_site_out; int *d_key_marks; tjamd_group_mark *d_marks; long mark_capacity, *h_n_marks;
};
struct MarkRefusal { const char *text; int value; };    // the message of an error bit ("%s" the entry, then "%d" the value where it has one)

// per_sample: the entry's array over the samples (d_group, d_order), and its name
static int mark_check_head (const MarkCall &m, const void *per_sample, const char *per_sample_name)
{
  if (!m.c) return set_err (TJAMD_ERR_ARG, "%s: null counter", m.fn);
  if (m.n_sites < 0) return set_err (TJAMD_ERR_ARG, "%s: n_sites %ld below 0", m.fn, m.n_sites);
  if (m.n_sites > 0 && (!m.d_sites || !m.d_genotype)) return set_err (TJAMD_ERR_ARG, "%s: null site or genotype buffer", m.fn);
  if (!per_sample) return set_err (TJAMD_ERR_ARG, "%s: null %s", m.fn, per_sample_name);
  if (m.n_samples < 1 || m.n_samples > CLD_MAX) return set_err (TJAMD_ERR_ARG, "%s: n_samples %d outside 1..4096", m.fn, m.n_samples);
  return 0;
}

// keys: the entry's noun for its keys; what: what the device does, for the message about a missing one
static int mark_check_tail (const MarkCall &m, const char *keys, const char *what)
{
  if (m.min_called < 1) return set_err (TJAMD_ERR_ARG, "%s: min_called %d below 1", m.fn, m.min_called);
  if (m.mark_capacity < 0) return set_err (TJAMD_ERR_ARG, "%s: mark_capacity %ld below 0", m.fn, m.mark_capacity);
  if (!m.d_marks && m.mark_capacity > 0) return set_err (TJAMD_ERR_ARG, "%s: null d_marks with a capacity of %ld", m.fn, m.mark_capacity);
  if (m.n_sites >= (1l << 31) || m.n_sites * (long) m.n_samples >= (1l << 31)) return set_err (TJAMD_ERR_ARG, "%s: %ld sites x %d samples: 2^31 cells or more", m.fn, m.n_sites, m.n_samples);
  if (m.d_calls && m.n_sites * (long) m.n_keys >= (1l << 31)) return set_err (TJAMD_ERR_ARG, "%s: %ld sites x %d %s: 2^31 calls or more", m.fn, m.n_sites, m.n_keys, keys);
  if (tjamd_device_count () <= 0) return set_err (TJAMD_ERR_NO_DEVICE, "%s: TJAMD_ERR_NO_DEVICE: no HIP device visible (%s on the device; no CPU fallback)", m.fn, what);
  return 0;
}

// The three steps of a checked call.  timer: the entry's stage; small: its wavefront form; refused: the messages of its error
// bits, the lowest first, ended by a null text; launch (A, emit, grid, per_block): a pass of its form, the first (emit false)
// or the second.  Returns what the entry returns.
template <class Launch>
static long mark_sites (const MarkCall &m, int timer, bool small, const MarkRefusal *refused, Launch launch)
{
  tjamd_counter *c = m.c;
  const char *fn = m.fn;
  Stage st (c, timer);                                  // (a call that returns no count leaves no timing behind)
  if (hipSetDevice (c->device) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
  int rc;
  if (m.n_sites == 0 || m.n_keys == 0) {                // no site or no key: no mark, no kernel
    if (m.d_key_marks && m.n_keys > 0 && hipMemsetAsync (m.d_key_marks, 0, (size_t) m.n_keys * sizeof (int), c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: memset failed", fn);
    rc = read_back (c, fn, nullptr, nullptr, 0);
    if (rc) return -rc;
    if (m.h_n_marks) *m.h_n_marks = 0;
    return 0;
  }
  ScratchCut cut;
  int *flags; u32 *cnt;
  cut.take (flags, (size_t) 64 + m.n_keys); cut.take (cnt, (size_t) m.n_sites);
  rc = cut.commit (c);
  if (!rc) rc = ensure (c->scan_tmp, scan_tmp_words (m.n_sites) * 4 + 64, c->stream);
  if (rc) return -rc;
  if (hipMemsetAsync (flags, 0, ((size_t) 64 + m.n_keys) * sizeof (int), c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: memset failed", fn);
  const MarkArgs A = {m.n_samples, m.n_keys, m.min_called, (const Site *) m.d_sites, m.n_sites, m.d_genotype, (GroupCall *) m.d_calls, (GroupSite *) m.d_site_out, m.d_key_marks,
                      (GroupMark *) m.d_marks, m.mark_capacity, flags, flags + 64, cnt};
  // the first form: wavefronts that take a site each in turn, CLD_WAVE_SITES / 4 or more a wavefront where there are that many; the second: two workgroups a CU, each a run of sites
  const long blocks = small ? std::max (1l, std::min ((m.n_sites + CLD_WAVE_SITES - 1) / CLD_WAVE_SITES, 8l * c->n_cu)) : std::min (m.n_sites, 2l * c->n_cu);
  const long per_block = (m.n_sites + blocks - 1) / blocks;
  const unsigned grid = (unsigned) (small ? blocks : (m.n_sites + per_block - 1) / per_block);
  st.begin ();
  launch (A, false, grid, per_block);
  rc = exclusive_scan (c, cnt, cnt, m.n_sites, (u32 *) flags + 1);
  if (rc) return -rc;
  launch (A, true, grid, per_block);
  st.end ();
  u32 h[2] = {0, 0};
  rc = read_back (c, fn, flags, h, 2);
  if (rc) return -rc;
  for (int bit = 0; refused[bit].text; bit++)
    if (h[0] >> bit & 1u) return -set_err (TJAMD_ERR_ARG, refused[bit].text, fn, refused[bit].value);
  if (m.h_n_marks) *m.h_n_marks = (long) h[1];
  if ((long) h[1] > m.mark_capacity) return -set_err (TJAMD_ERR_CAPACITY, "%s: %u marks, caller capacity %ld", fn, h[1], m.mark_capacity);
  st.done ();
  return (long) h[1];
}

extern "C" long tjamd_group_sites (tjamd_counter *c, const tjamd_site *d_sites, long n_sites, const int16_t *d_genotype, int n_samples, const int *d_group, int n_groups,
                                   int min_called, tjamd_group_call *d_calls, tjamd_group_site *d_site_out, int *d_group_marks, tjamd_group_mark *d_marks, long mark_capacity,
                                   long *h_n_marks)
{
  const MarkCall m = {"tjamd_group_sites", c, d_sites, n_sites, d_genotype, n_samples, n_groups, min_called, d_calls, d_site_out, d_group_marks, d_marks, mark_capacity, h_n_marks};
  int rc = mark_check_head (m, d_group, "d_group");
  if (rc) return -rc;
  if (n_groups < 1 || n_groups > CLD_MAX) return -set_err (TJAMD_ERR_ARG, "%s: n_groups %d outside 1..4096", m.fn, n_groups);
  rc = mark_check_tail (m, "groups", "the sites are read by group");
  if (rc) return -rc;
  const bool small = n_samples <= CLD_SMALL && c->groups_small;
  const MarkRefusal refused[] = {{"%s: a label is below -1 or not below n_groups %d", n_groups}, {"%s: a site has n_alleles < 1 or above n_samples %d", n_samples},
                                 {"%s: a genotype cell is below -1 or above its site's n_alleles", 0}, {nullptr, 0}};
  return mark_sites (m, T_GROUP_SITES, small, refused, [&] (const MarkArgs &M, bool emit, unsigned grid, long per_block) {
    const GroupArgs A = {M, d_group};
    if (small && !emit) hipLaunchKernelGGL (group_sites_small_kernel<false>, dim3 (grid), dim3 (256), 0, c->stream, A);
    else if (small) hipLaunchKernelGGL (group_sites_small_kernel<true>, dim3 (grid), dim3 (256), 0, c->stream, A);
    else if (!emit) hipLaunchKernelGGL (group_sites_large_kernel<false>, dim3 (grid), dim3 (CLD_THREADS), 0, c->stream, A, per_block);
    else hipLaunchKernelGGL (group_sites_large_kernel<true>, dim3 (grid), dim3 (CLD_THREADS), 0, c->stream, A, per_block);
  });
}
TJ_LAST_MS (tjamd_last_group_sites_ms, T_GROUP_SITES)

// ---- N17: the tree of the links as nodes, and the sites that support each of its clades ------------------------------------
// The rules as built are in include/tatajuba_clades.h.
// linkage_tree_kernel: one workgroup.  All lanes check the ends of every link and pack them into LDS; lane 0 then steps through
//   the links in their order with a union-find in LDS whose root is always its component's smallest member (path halving), so
//   that `left` needs no second table, and writes children and sizes into LDS; a cycle ends the walk.  Both checks come before
//   any store to the caller.  The roots, ascending, are the samples that are their own label: a scan of their sizes lays them
//   out; lane 0 walks the nodes from the last to the first and hands each child its first position, a leaf its place in the
//   order.  The walk of one lane is the cost of the call; a tree is built once.
// clade_sites: N16's three steps (a pass that checks and counts, the shared scan, the same kernel compiled with the stores),
//   with the clade as the group.  A clade is an interval of the leaf order, so a node's record comes from prefix counts over
//   that order and costs the same at any depth of the tree:
//   up to 64 samples, clade_sites_small_kernel: a wavefront per site, a lane per leaf position, then a lane per node.  Per
//     site the ballot of the called positions, per lane the number of called samples that carry its genotype, and the ballot
//     of the change points (a called position whose genotype differs from the nearest called one before it).  A node's called
//     members are called & its interval mask; its genotype is that of their first position p0, fixed iff no change point lies
//     behind p0 inside the interval; both come to the node's lane by one exchange each.  The nodes' intervals sit packed in
//     LDS, made once per workgroup.
//   beyond, clade_sites_large_kernel: a workgroup of 1024 walks a run of sites, four consecutive positions a thread.  A scan
//     of the called flags gives pc[p], the called samples before p, and compacts the called genotypes into gc[rank] in leaf
//     order; a second scan over the ranks counts the change points up to each rank (kr).  Node j with the interval [f, f + n):
//     r0 = pc[f], r1 = pc[f + n], n_called = r1 - r0, its genotype gc[r0], fixed iff kr[r1 - 1] == kr[r0].  The carriers of
//     a genotype are counted as in N16 (LDS atomics behind a fold of equal lanes), the marks of 64 nodes are a ballot word.
// Global atomics: the error flag, and a node's marks once per workgroup into scratch (the small form: once per mark for the
// nodes from the 64th on, which a tree of 64 samples does not have).

struct TreeNode { int left, right, first, size; };
static_assert (sizeof (TreeNode) == 16 && sizeof (TreeNode) == sizeof (tjamd_tree_node), "tree node layout");
// a caller's node lies inside the ns samples: an interval [first, first + size) of the leaf order with two members or more
__device__ __forceinline__ bool tree_node_ok (const TreeNode &nd, int ns) { return nd.size >= 2 && nd.size <= ns && nd.first >= 0 && nd.first <= ns - nd.size; }

__device__ __forceinline__ void linkage_tree_body (const Link *__restrict__ links, int n_links, int ns, TreeNode *__restrict__ nodes, int *__restrict__ order, int *__restrict__ flags)
{
  __shared__ int uf[CLD_MAX], cnode[CLD_MAX];           // a sample's label; per root (its component's smallest member) the node that is the component, or -1 - sample
  __shared__ int nl[CLD_MAX], nr[CLD_MAX], nsz[CLD_MAX], nfi[CLD_MAX];   // the nodes; nfi: a link's packed ends on the way up, a node's first position on the way down
  __shared__ int wsum[16];
  __shared__ int s_cycle;
  const int tid = threadIdx.x;
  int bad = 0;
  for (int j = tid; j < n_links; j += 1024) {
    const Link l = links[j];
    const bool ok = l.a >= 0 && l.a < l.b && l.b < ns;
    if (!ok) bad = 1;
    nfi[j] = ok ? (l.a | l.b << 16) : 0;
  }
  for (int v = tid; v < ns; v += 1024) { uf[v] = v; cnode[v] = -1 - v; }
  if (tid == 0) s_cycle = 0;
  if (__syncthreads_or (bad)) { if (tid == 0) flags[0] = 1; return; }
  if (tid == 0)
    for (int j = 0; j < n_links; j++) {
      int ra = nfi[j] & 0xffff, rb = nfi[j] >> 16;
      while (uf[ra] != ra) { const int up = uf[uf[ra]]; uf[ra] = up; ra = up; }
      while (uf[rb] != rb) { const int up = uf[uf[rb]]; uf[rb] = up; rb = up; }
      if (ra == rb) { s_cycle = 1; break; }
      const int lo = min (ra, rb), hi = max (ra, rb), cl = cnode[lo], cr = cnode[hi];
      nl[j] = cl; nr[j] = cr; nsz[j] = (cl >= 0 ? nsz[cl] : 1) + (cr >= 0 ? nsz[cr] : 1);
      uf[hi] = lo; cnode[lo] = j;
    }
  __syncthreads ();
  if (s_cycle) { if (tid == 0) flags[0] = 2; return; }
  // the roots in the order of their smallest member, four consecutive samples a thread
  int mine = 0;
  #pragma unroll
  for (int j = 0; j < CLD_PER; j++) {
    const int v = CLD_PER * tid + j;
    if (v < ns && uf[v] == v) mine += cnode[v] >= 0 ? nsz[cnode[v]] : 1;
  }
  int n_leaves;                                         // (ns: every sample is under one root)
  int at = block_exclusive_scan_1024 (mine, tid, wsum, n_leaves);
  #pragma unroll
  for (int j = 0; j < CLD_PER; j++) {
    const int v = CLD_PER * tid + j;
    if (v < ns && uf[v] == v) {
      const int cn = cnode[v];
      if (cn >= 0) { nfi[cn] = at; at += nsz[cn]; } else order[at++] = v;
    }
  }
  __syncthreads ();
  if (tid == 0)
    for (int j = n_links - 1; j >= 0; j--) {            // a parent comes before its children
      const int f = nfi[j], l = nl[j], r = nr[j], fr = f + (l >= 0 ? nsz[l] : 1);
      if (l >= 0) nfi[l] = f; else order[f] = -1 - l;
      if (r >= 0) nfi[r] = fr; else order[fr] = -1 - r;
    }
  __syncthreads ();
  for (int j = tid; j < n_links; j += 1024) nodes[j] = TreeNode {nl[j], nr[j], nfi[j], nsz[j]};
}
__global__ __launch_bounds__ (1024)
void linkage_tree_kernel (const Link *__restrict__ links, int n_links, int ns, TreeNode *__restrict__ nodes, int *__restrict__ order, int *__restrict__ flags)
{ linkage_tree_body (links, n_links, ns, nodes, order, flags); }

extern "C" long tjamd_linkage_tree (tjamd_counter *c, const tjamd_link *d_links, long n_links, int n_samples, tjamd_tree_node *d_nodes, int *d_order)
{
  static const char *fn = "tjamd_linkage_tree";
  if (!c) return -set_err (TJAMD_ERR_ARG, "%s: null counter", fn);
  if (!d_order) return -set_err (TJAMD_ERR_ARG, "%s: null d_order", fn);
  if (n_samples < 1 || n_samples > CLD_MAX) return -set_err (TJAMD_ERR_ARG, "%s: n_samples %d outside 1..4096", fn, n_samples);
  if (n_links < 0 || n_links > n_samples - 1) return -set_err (TJAMD_ERR_ARG, "%s: n_links %ld outside 0..n_samples - 1 = %d", fn, n_links, n_samples - 1);
  if (n_links > 0 && (!d_links || !d_nodes)) return -set_err (TJAMD_ERR_ARG, "%s: null link or node buffer", fn);
  Stage st (c, T_LINKAGE_TREE);                         // (a refused call leaves no timing behind)
  if (const int bad = st.enter (fn, "the tree is built")) return -bad;
  ScratchCut cut;
  int *flags;
  int rc = commit_with_flags (cut, c, fn, flags);
  if (rc) return -rc;
  st.begin ();
  hipLaunchKernelGGL (linkage_tree_kernel, dim3 (1), dim3 (1024), 0, c->stream, (const Link *) d_links, (int) n_links, n_samples, (TreeNode *) d_nodes, d_order, flags);
  st.end ();
  u32 h_flags[1] = {0};
  rc = read_back (c, fn, flags, h_flags, 1);
  if (rc) return -rc;
  if (h_flags[0] == 1) return -set_err (TJAMD_ERR_ARG, "%s: a link has a < 0, a >= b or b >= n_samples", fn);
  if (h_flags[0] == 2) return -set_err (TJAMD_ERR_ARG, "%s: a link joins two samples that the links before it have joined: a cycle", fn);
  st.done ();
  return n_links;
}
TJ_LAST_MS (tjamd_last_linkage_tree_ms, T_LINKAGE_TREE)

struct CladeArgs : MarkArgs { const TreeNode *nodes; const int *order; };   // (the words of a call: at MarkArgs)

template <bool EMIT>
__global__ __launch_bounds__ (256)
void clade_sites_small_kernel (const CladeArgs A)
{
  __shared__ int s_node[CLD_MAX];                       // first | size << 8 of every node (both at most 64); 0: no node, or a refused one
  __shared__ int s_seen[4][CLD_SMALL], s_marks[4][CLD_SMALL];
  if (EMIT && !marks_emit_begin<256> (A)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ns = A.ns, n_nodes = A.n_keys;
  int bad = 0, my_marks = 0;
  for (int j = tid; j < n_nodes; j += 256) {
    const TreeNode nd = A.nodes[j];
    const bool ok = tree_node_ok (nd, ns);
    if (!ok) bad |= 2;
    s_node[j] = ok ? (nd.first | nd.size << 8) : 0;
  }
  int smp = lane;                                       // the sample at this lane's leaf position
  if (lane < ns) {
    smp = A.order[lane];
    if (smp < 0 || smp >= ns) { bad |= 1; smp = lane; }
  }
  s_seen[wave][lane] = 0;
  __syncthreads ();
  if (lane < ns) s_seen[wave][smp] = 1;
  __syncthreads ();
  if (lane < ns && !s_seen[wave][lane]) bad |= 1;       // ns positions on ns samples: one sample left out is one sample twice
  const u64 below = (1ull << lane) - 1ull;
  for (long i = (long) blockIdx.x * 4 + wave; i < A.n_sites; i += (long) gridDim.x * 4) {
    const int na = A.sites[i].n_alleles;
    if (na < 1 || na > ns) {                            // (the whole wavefront)
      bad |= 4;
      if (!EMIT && lane == 0) A.cnt[i] = 0;
      continue;
    }
    int g = -1;
    if (lane < ns) {
      g = A.geno[i * ns + smp];
      if (g < -1 || g > na) { bad |= 8; g = -1; }
    }
    const u64 called = __ballot (g >= 0);
    const int all_called = __popcll (called);
    int carriers = 0, n_genotypes = 0;                  // the called samples that carry this lane's genotype; one step per distinct genotype
    for (u64 rem = called; rem; n_genotypes++) {
      const u64 m = __ballot (g == __builtin_amdgcn_readlane (g, __ffsll ((long long) rem) - 1));
      if ((m >> lane) & 1ull) carriers = __popcll (m);
      rem &= ~m;
    }
    const u64 before = called & below;
    const int prev = __shfl (g, before ? 63 - __clzll ((long long) before) : lane);
    const u64 change = __ballot (g >= 0 && before != 0 && prev != g);
    const long at = EMIT ? (long) A.cnt[i] : 0;
    int n_marks = 0, first = -1;
    for (int base = 0; base < n_nodes; base += 64) {    // a lane per node
      const int j = base + lane, v = j < n_nodes ? s_node[j] : 0, f = v & 0xff, sz = v >> 8;
      const u64 mask = sz == 0 ? 0ull : (sz >= 64 ? ~0ull : (1ull << sz) - 1ull) << f, cm = called & mask;
      const int p0 = cm ? __ffsll ((long long) cm) - 1 : 0;
      const int x = __shfl (g, p0), nx = __shfl (carriers, p0);   // (every lane takes part in every exchange)
      GroupCall q = {(int) __popcll (cm), -1, 0, 0};
      if (cm) {
        q.fixed = (change & mask & ~((2ull << p0) - 1ull)) ? -2 : x;
        if (q.fixed >= 0) {
          q.n_outside = nx - q.n_called;
          q.mark = mark_rule (q.n_called, A.min_called, q.n_outside, all_called > q.n_called);
        }
      }
      if (EMIT && A.calls && j < n_nodes) A.calls[i * n_nodes + j] = q;
      const u64 mb = __ballot (q.mark != 0);
      if (mb) {
        if (first < 0) first = base + __ffsll ((long long) mb) - 1;
        if (q.mark) {
          if (EMIT) {
            const long pos = at + n_marks + __popcll (mb & below);
            if (A.marks && pos < A.cap) A.marks[pos] = GroupMark {(int) i, j, q.fixed, q.n_called};
          }
          else if (base == 0) my_marks++;
          else atomicAdd (&A.km[j], 1);
        }
        n_marks += __popcll (mb);
      }
    }
    if (!EMIT) {
      if (lane == 0) A.cnt[i] = (u32) n_marks;
      continue;
    }
    if (A.site_out && lane == 0) A.site_out[i] = GroupSite {all_called, n_genotypes, n_marks, first};
  }
  if (!EMIT) marks_count_end_small (A, bad, s_marks, my_marks, min (n_nodes, 64), tid);
}

template <bool EMIT>
__global__ __launch_bounds__ (CLD_THREADS)
void clade_sites_large_kernel (const CladeArgs A, long per_block)
{
  __shared__ int pc[CLD_MAX + 1], gc[CLD_MAX], kr[CLD_MAX], x_cnt[CLD_MAX + 1];
  __shared__ u64 markbits[CLD_MAX / 64];
  __shared__ int wsum[2][CLD_THREADS / 64];
  __shared__ int s_ngeno;
  if (EMIT && !marks_emit_begin<CLD_THREADS> (A)) return;
  const int tid = threadIdx.x, lane = tid & 63, ns = A.ns, n_nodes = A.n_keys;
  int bad = 0, smp[CLD_PER], node[CLD_PER], nmarks[CLD_PER];   // node: first | size << 16; 0: no node, or a refused one
  #pragma unroll
  for (int k = 0; k < CLD_PER; k++) {
    const int p = CLD_PER * tid + k, j = tid + CLD_THREADS * k;   // a thread's leaf positions are consecutive, its nodes a workgroup apart
    smp[k] = p; node[k] = 0; nmarks[k] = 0;
    if (p < ns) {
      smp[k] = A.order[p];
      if (smp[k] < 0 || smp[k] >= ns) { bad |= 1; smp[k] = p; }
    }
    if (j < n_nodes) {
      const TreeNode nd = A.nodes[j];
      if (tree_node_ok (nd, ns)) node[k] = nd.first | nd.size << 16;
      else bad |= 2;
    }
    x_cnt[j] = 0;
  }
  if (tid < CLD_MAX / 64) markbits[tid] = 0;
  if (tid == 0) { x_cnt[CLD_MAX] = 0; s_ngeno = 0; }
  __syncthreads ();
  #pragma unroll
  for (int k = 0; k < CLD_PER; k++)
    if (CLD_PER * tid + k < ns) x_cnt[smp[k]] = 1;
  __syncthreads ();
  #pragma unroll
  for (int k = 0; k < CLD_PER; k++) {                   // ns positions on ns samples: one sample left out is one sample twice
    const int j = tid + CLD_THREADS * k;
    if (j < ns && !x_cnt[j]) bad |= 1;
    x_cnt[j] = 0;
  }
  __syncthreads ();
  const long i0 = (long) blockIdx.x * per_block, i1 = min (A.n_sites, i0 + per_block);
  for (long i = i0; i < i1; i++) {
    const int na = A.sites[i].n_alleles;
    if (na < 1 || na > ns) {                            // (the whole workgroup; the tables are clean)
      bad |= 4;
      if (!EMIT && tid == 0) A.cnt[i] = 0;
      continue;
    }
    int g[CLD_PER], mine = 0;
    #pragma unroll
    for (int k = 0; k < CLD_PER; k++) {
      const int p = CLD_PER * tid + k;
      g[k] = -1;
      if (p < ns) {
        g[k] = A.geno[i * ns + smp[k]];
        if (g[k] < -1 || g[k] > na) { bad |= 8; g[k] = -1; }
      }
      mine += g[k] >= 0;
    }
    int all_called;
    int r = block_exclusive_scan_1024 (mine, tid, wsum[0], all_called);
    #pragma unroll
    for (int k = 0; k < CLD_PER; k++) {
      const int p = CLD_PER * tid + k;
      if (p < ns) {
        pc[p] = r;
        if (g[k] >= 0) gc[r++] = g[k];
      }
    }
    if (tid == 0) pc[ns] = all_called;
    if (CLD_PER * (tid & ~63) < ns) {                   // (a whole wavefront)
      const u64 packed = (u64) (g[0] + 1) | (u64) (g[1] + 1) << 16 | (u64) (g[2] + 1) << 32 | (u64) (g[3] + 1) << 48;   // (one body for the four)
      static_assert (CLD_PER == 4, "four genotypes in a word");
      #pragma unroll 1
      for (int k = 0; k < CLD_PER; k++) {
        const int gk = (int) ((packed >> (16 * k)) & 0xffffull) - 1;
        fold_equal_keys (gk >= 0, gk, lane, [&] (int n) { atomicAdd (&x_cnt[gk], n); });   // the carriers of the site's genotypes
      }
    }
    __syncthreads ();
    u32 ch = 0;                                         // bit k: a change point, a called rank whose genotype differs from the rank before it
    #pragma unroll
    for (int k = 0; k < CLD_PER; k++) {
      const int rr = CLD_PER * tid + k;
      ch |= (u32) (rr >= 1 && rr < all_called && gc[rr] != gc[rr - 1]) << k;
    }
    int all_changes;
    int kb = block_exclusive_scan_1024 (__popc (ch), tid, wsum[1], all_changes);
    #pragma unroll
    for (int k = 0; k < CLD_PER; k++) {
      const int rr = CLD_PER * tid + k;
      kb += (ch >> k) & 1u;
      if (rr < all_called) kr[rr] = kb;
    }
    __syncthreads ();
    u32 marked = 0;                                     // bit k: this thread's k-th node is marked here
    #pragma unroll 1
    for (int k = 0; k < CLD_PER; k++) {                 // a thread per node, one body for the four
      const int j = tid + CLD_THREADS * k, nd = k == 0 ? node[0] : k == 1 ? node[1] : k == 2 ? node[2] : node[3];
      if (CLD_THREADS * k + (tid & ~63) >= n_nodes) break;   // (a whole wavefront)
      int nc = 0, fixed = -1, n_outside = 0, mark = 0;
      if (nd) {
        const int r0 = pc[nd & 0xffff], r1 = pc[(nd & 0xffff) + (nd >> 16)];
        nc = r1 - r0;
        if (nc) {
          const int x = gc[r0];
          fixed = kr[r1 - 1] != kr[r0] ? -2 : x;
          if (fixed >= 0) {
            n_outside = x_cnt[x] - nc;
            mark = mark_rule (nc, A.min_called, n_outside, all_called > nc);
          }
        }
      }
      if (EMIT && A.calls && j < n_nodes) A.calls[i * n_nodes + j] = GroupCall {nc, fixed, n_outside, mark};
      const u64 mb = __ballot (mark != 0);
      if (lane == 0) markbits[j >> 6] = mb;
      if (!EMIT) { nmarks[0] += mark & (k == 0); nmarks[1] += mark & (k == 1); nmarks[2] += mark & (k == 2); nmarks[3] += mark & (k == 3); }
      marked |= (u32) mark << k;
    }
    if (EMIT && A.site_out) {                           // site_count_genotypes (), written out: through the helper this kernel takes 65 registers, one more than eight wavefronts a SIMD have
      int nzx = 0;
      for (int x = tid; x <= na; x += CLD_THREADS) nzx += x_cnt[x] != 0;
      for (int o = 32; o; o >>= 1) nzx += __shfl_xor (nzx, o);
      if (nzx && lane == 0) atomicAdd (&s_ngeno, nzx);
    }
    __syncthreads ();
    site_marks_total<EMIT> (A, i, markbits, tid, all_called, s_ngeno, [&] { s_ngeno = 0; });
    if (EMIT && marked && A.marks) {
      #pragma unroll 1
      for (int k = 0; k < CLD_PER; k++) {
        if (!((marked >> k) & 1u)) continue;
        const int j = tid + CLD_THREADS * k, nd = k == 0 ? node[0] : k == 1 ? node[1] : k == 2 ? node[2] : node[3];
        const int r0 = pc[nd & 0xffff], r1 = pc[(nd & 0xffff) + (nd >> 16)];   // (the site's tables stand until the next barrier)
        const long pos = site_mark_place (A, i, markbits, j);
        if (pos < A.cap) A.marks[pos] = GroupMark {(int) i, j, gc[r0], r1 - r0};
      }
    }
    site_clear_genotypes (x_cnt, na, tid);
    __syncthreads ();
  }
  if (!EMIT) marks_count_end (A, bad, nmarks, tid);
}

extern "C" long tjamd_clade_sites (tjamd_counter *c, const tjamd_site *d_sites, long n_sites, const int16_t *d_genotype, int n_samples, const tjamd_tree_node *d_nodes, int n_nodes,
                                   const int *d_order, int min_called, tjamd_group_call *d_calls, tjamd_group_site *d_site_out, int *d_node_marks, tjamd_group_mark *d_marks,
                                   long mark_capacity, long *h_n_marks)
{
  const MarkCall m = {"tjamd_clade_sites", c, d_sites, n_sites, d_genotype, n_samples, n_nodes, min_called, d_calls, d_site_out, d_node_marks, d_marks, mark_capacity, h_n_marks};
  int rc = mark_check_head (m, d_order, "d_order");
  if (rc) return -rc;
  if (n_nodes < 0 || n_nodes > CLD_MAX) return -set_err (TJAMD_ERR_ARG, "%s: n_nodes %d outside 0..4096", m.fn, n_nodes);
  if (!d_nodes && n_nodes > 0) return -set_err (TJAMD_ERR_ARG, "%s: null d_nodes", m.fn);
  rc = mark_check_tail (m, "nodes", "the sites are read by clade");
  if (rc) return -rc;
  const bool small = n_samples <= CLD_SMALL && c->clades_small;
  const MarkRefusal refused[] = {{"%s: d_order is not a permutation of 0 .. n_samples - 1", 0}, {"%s: a node has size < 2, first < 0 or first + size above n_samples %d", n_samples},
                                 {"%s: a site has n_alleles < 1 or above n_samples %d", n_samples}, {"%s: a genotype cell is below -1 or above its site's n_alleles", 0}, {nullptr, 0}};
  return mark_sites (m, T_CLADE_SITES, small, refused, [&] (const MarkArgs &M, bool emit, unsigned grid, long per_block) {
    const CladeArgs A = {M, (const TreeNode *) d_nodes, d_order};
    if (small && !emit) hipLaunchKernelGGL (clade_sites_small_kernel<false>, dim3 (grid), dim3 (256), 0, c->stream, A);
    else if (small) hipLaunchKernelGGL (clade_sites_small_kernel<true>, dim3 (grid), dim3 (256), 0, c->stream, A);
    else if (!emit) hipLaunchKernelGGL (clade_sites_large_kernel<false>, dim3 (grid), dim3 (CLD_THREADS), 0, c->stream, A, per_block);
    else hipLaunchKernelGGL (clade_sites_large_kernel<true>, dim3 (grid), dim3 (CLD_THREADS), 0, c->stream, A, per_block);
  });
}
TJ_LAST_MS (tjamd_last_clade_sites_ms, T_CLADE_SITES)

// ---- N18: complete and average linkage trees of the samples ------------------------------------------------------------------
// N14's sample x sample matrix agglomerated under complete or average linkage by rounds of reciprocal nearest neighbours; the
// rule as built is in include/tatajuba_agglomerate.h.  Not a spanning forest: the cluster x cluster matrix is rewritten as
// clusters merge, in place, in the u64 key matrix of N15's key pass (the maximum, or the exact sum, of the pairs across two
// clusters; all ones: no edge, which absorbs).
//   1. linkage_keys_kernel as N15 runs it, then aggl_init_kernel: every sample a cluster of size 1, and under AVERAGE the bound
//      of 2^40 on a key.  Raises the error flag; writes nothing of the caller's.
//   2. rounds of four kernels, launched in batches of AGGL_BATCH without a look at the device in between:
//      (a) aggl_rowmin_kernel: a wavefront per live row takes the minimum of (D, id) over the live columns; under AVERAGE D is
//          the cell's sum divided by the two sizes, taken here and never stored.
//      (b) aggl_pairs_kernel, one workgroup with the nearest neighbours in LDS: the mutual pairs, their links with the round,
//          the round's pair list, the new sizes (no other kernel of the round reads a size of a cluster that merges: the update
//          needs the pair list alone); `done` when no pair is left or the tree is whole.
//      (c) aggl_rows_kernel, a workgroup per pair (X, Y): row X := f (row X, row Y) over all columns; then aggl_cols_kernel, a
//          wavefront per live row: column P := f (column P, column Q) for every pair (P, Q).  The second reads what the first
//          wrote, so the cell (X, P) of two pairs of one round holds f of all four cells, and the matrix stays symmetric.
//      Every kernel of a round returns when `done` or the error flag is up.  Nothing waits for another workgroup.
//   3. aggl_sort_kernel, behind every batch, returns unless `done` is up: one workgroup sorts the links by (key, round, a, b)
//      in LDS (two u64 per entry, 64 KB at 4096 places) and stores them.
// Up to 64 samples aggl_small_kernel does all of it as one workgroup in one launch, the matrix in LDS.  DESIGN.md section 3.5, N18.

struct AgglEdge { u64 key, aux; };                      // a link before the sort: aux = round << 24 | a << 12 | b, a < b < 4096, round < 4096
#define AGGL_BATCH 32                                   // rounds enqueued between two looks at the flag words (measured)
#define AGGL_KEY_MAX (1ull << 40)                       // AVERAGE: a key of a pair of samples stays below this, a sum over 2^22 pairs below 2^62
// flags of a call: [0] error bits (1 a cell's values, 2 a cell and its mirror, 4 a key of 2^40 or more under AVERAGE), [1] done,
// [2] links appended so far, [3] rounds that merged something, [4] the pairs of the last round

__device__ __forceinline__ u64 aggl_f (u64 x, u64 y, int linkage)
{
  if (x == LINK_NONE || y == LINK_NONE) return LINK_NONE;
  return linkage == TJAMD_AGGL_COMPLETE ? (x > y ? x : y) : x + y;
}
// the distance of two clusters from their cell (not LINK_NONE) and their sizes
__device__ __forceinline__ u64 aggl_d (u64 cell, int sa, int sb, int linkage)
{ // (sa + sb <= 4096: the product is below 2^23; dividing by it is floor (floor (S / sb) / sa))
  const u32 pairs = (u32) sa * (u32) sb;
  return linkage == TJAMD_AGGL_COMPLETE || pairs == 1u ? cell : cell / (u64) pairs;
}

__global__ __launch_bounds__ (256)
void aggl_init_kernel (const u64 *__restrict__ keys, int ns, int ld, int linkage, int *__restrict__ size, int *__restrict__ flags)
{
  const long n = (long) ns * ld, x0 = (long) blockIdx.x * 256 + threadIdx.x;
  if (x0 < ld) size[x0] = x0 < ns ? 1 : 0;              // (the padding column is a retired cluster)
  if (linkage != TJAMD_AGGL_AVERAGE) return;
  int bad = 0;
  for (long x = x0; x < n; x += (long) gridDim.x * 256) {
    const u64 k = keys[x];
    if (k != LINK_NONE && k >= AGGL_KEY_MAX) bad = 4;
  }
  if (bad) atomicOr (flags, bad);
}

__device__ __forceinline__ void aggl_rowmin_body (const u64 *__restrict__ keys, int ns, int ld, int linkage, const int *__restrict__ size, LinkRowBest *__restrict__ rowbest,
                         const int *__restrict__ flags)
{
  if (link_rounds_over (flags)) return;
  const int lane = threadIdx.x & 63, a = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (a >= ns) return;                                  // (a whole wavefront)
  const int sa = size[a];
  if (sa == 0) return;                                  // a retired row
  const ulonglong2 *row = (const ulonglong2 *) (keys + (long) a * ld);   // (ld is even and the matrix starts on a 256-byte boundary: 16-byte loads)
  const int2 *size2 = (const int2 *) size;
  u64 bk = LINK_NONE;
  int bb = 0x7fffffff;
  #pragma unroll 2
  for (int p = lane; p < ld / 2; p += 64) {             // (a lane's b ascend: the first of equal distances stays; the diagonal holds LINK_NONE)
    const ulonglong2 k = row[p];
    const int2 sb = size2[p];
    if (sb.x != 0 && k.x != LINK_NONE) { const u64 d = aggl_d (k.x, sa, sb.x, linkage); if (d < bk) { bk = d; bb = 2 * p; } }
    if (sb.y != 0 && k.y != LINK_NONE) { const u64 d = aggl_d (k.y, sa, sb.y, linkage); if (d < bk) { bk = d; bb = 2 * p + 1; } }
  }
  wave_min_key_b (bk, bb);
  if (lane == 0) rowbest[a] = LinkRowBest {bk, bb, 0};
}
__global__ __launch_bounds__ (256)
void aggl_rowmin_kernel (const u64 *__restrict__ keys, int ns, int ld, int linkage, const int *__restrict__ size, LinkRowBest *__restrict__ rowbest,
                         const int *__restrict__ flags)
{ aggl_rowmin_body (keys, ns, ld, linkage, size, rowbest, flags); }

__device__ __forceinline__ void aggl_pairs_body (const LinkRowBest *__restrict__ rowbest, int ns, int *__restrict__ size, AgglEdge *__restrict__ edges, u32 *__restrict__ pairs, int *__restrict__ flags)
{
  __shared__ int nn[LINK_MAX];                          // a live cluster's nearest neighbour; -1: retired, or no edge
  __shared__ int n_new;
  if (link_rounds_over (flags)) return;
  const int tid = threadIdx.x, base = flags[2], round = flags[3];
  u64 key[LINK_MAX / 1024];
  int sv[LINK_MAX / 1024];
  #pragma unroll
  for (int j = 0; j < LINK_MAX / 1024; j++) {
    const int v = tid + 1024 * j;
    key[j] = LINK_NONE; sv[j] = 0;
    if (v < ns) {
      sv[j] = size[v];
      if (sv[j] != 0) { const LinkRowBest rb = rowbest[v]; key[j] = rb.key; nn[v] = rb.key != LINK_NONE ? rb.b : -1; }
      else nn[v] = -1;
    }
  }
  if (tid == 0) n_new = 0;
  __syncthreads ();
  #pragma unroll
  for (int j = 0; j < LINK_MAX / 1024; j++) {
    const int v = tid + 1024 * j;
    if (v >= ns || key[j] == LINK_NONE) continue;
    const int w = nn[v];
    if (w > v && nn[w] == v) {                          // mutual: one link, from its smaller end (fewer than ns links in all)
      const int at = atomicAdd (&n_new, 1);
      edges[base + at] = AgglEdge {key[j], (u64) round << 24 | (u64) v << 12 | (u64) w};
      pairs[at] = (u32) v << 12 | (u32) w;
      size[v] = sv[j] + size[w]; size[w] = 0;           // (v and w are in this pair alone)
    }
  }
  __syncthreads ();
  if (tid == 0) {
    if (n_new == 0) flags[1] = 1;                       // no live cluster has an edge
    else {
      flags[2] = base + n_new; flags[3] = round + 1; flags[4] = n_new;
      if (base + n_new == ns - 1) flags[1] = 1;         // one cluster is left: the matrix is not needed again
    }
  }
}
__global__ __launch_bounds__ (1024)
void aggl_pairs_kernel (const LinkRowBest *__restrict__ rowbest, int ns, int *__restrict__ size, AgglEdge *__restrict__ edges, u32 *__restrict__ pairs, int *__restrict__ flags)
{ aggl_pairs_body (rowbest, ns, size, edges, pairs, flags); }

__device__ __forceinline__ void aggl_rows_body (u64 *__restrict__ keys, int ld, int linkage, const u32 *__restrict__ pairs, const int *__restrict__ flags)
{
  if (link_rounds_over (flags)) return;
  if ((int) blockIdx.x >= flags[4]) return;
  const u32 pair = pairs[blockIdx.x];
  ulonglong2 *rx = (ulonglong2 *) (keys + (long) (pair >> 12) * ld);
  const ulonglong2 *ry = (const ulonglong2 *) (keys + (long) (pair & 4095u) * ld);
  for (int p = threadIdx.x; p < ld / 2; p += 256) {
    const ulonglong2 x = rx[p], y = ry[p];
    rx[p] = ulonglong2 {aggl_f (x.x, y.x, linkage), aggl_f (x.y, y.y, linkage)};
  }
}
__global__ __launch_bounds__ (256)
void aggl_rows_kernel (u64 *__restrict__ keys, int ld, int linkage, const u32 *__restrict__ pairs, const int *__restrict__ flags)
{ aggl_rows_body (keys, ld, linkage, pairs, flags); }

__device__ __forceinline__ void aggl_cols_body (u64 *__restrict__ keys, int ns, int ld, int linkage, const int *__restrict__ size, const u32 *__restrict__ pairs, const int *__restrict__ flags)
{
  if (link_rounds_over (flags)) return;
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= ns || size[r] == 0) return;                  // (a whole wavefront) a retired row is not read again
  u64 *row = keys + (long) r * ld;
  const int n = flags[4];
  for (int i = lane; i < n; i += 64) {                  // (the pairs of a round share no cluster: no cell is written twice)
    const u32 pair = pairs[i];
    const int P = (int) (pair >> 12), Q = (int) (pair & 4095u);
    row[P] = aggl_f (row[P], row[Q], linkage);
  }
}
__global__ __launch_bounds__ (256)
void aggl_cols_kernel (u64 *__restrict__ keys, int ns, int ld, int linkage, const int *__restrict__ size, const u32 *__restrict__ pairs, const int *__restrict__ flags)
{ aggl_cols_body (keys, ns, ld, linkage, size, pairs, flags); }

__device__ __forceinline__ void aggl_sort_body (const AgglEdge *__restrict__ edges, int P, Link *__restrict__ out, const int *__restrict__ flags)
{
  __shared__ u64 skey[LINK_MAX], saux[LINK_MAX];        // (64 KB: nothing else is in LDS here)
  if (((volatile const int *) flags)[0] != 0 || ((volatile const int *) flags)[1] == 0) return;
  const int tid = threadIdx.x, n = flags[2];            // (n <= P, a power of two up to LINK_MAX)
  for (int i = tid; i < P; i += 1024) {
    const bool in = i < n;
    skey[i] = in ? edges[i].key : LINK_NONE; saux[i] = in ? edges[i].aux : LINK_NONE;
  }
  __syncthreads ();
  lds_bitonic_sort<1024> (skey, saux, P);
  for (int i = tid; i < n; i += 1024) out[i] = Link {(int) (saux[i] >> 12 & 4095u), (int) (saux[i] & 4095u), (long long) skey[i]};
}
__global__ __launch_bounds__ (1024)
void aggl_sort_kernel (const AgglEdge *__restrict__ edges, int P, Link *__restrict__ out, const int *__restrict__ flags)
{ aggl_sort_body (edges, P, out, flags); }

// Up to LINK_SMALL samples: the checks, the rounds and the sort as one workgroup in one launch, the matrix in LDS (32 KB).
// Waves take the rows in turn for the row minimum; thread v is sample v when the pairs are found; the two phases of the update
// are two loops with a barrier between them.
// The body, as linkage_small_body: -> the number of links, or -1; `rounds`: the rounds that merged something
__device__ __forceinline__ int aggl_small_body (const SampleDistance *__restrict__ dist, int ns, int metric, int min_both, int linkage, Link &mine, int &rounds, int &bad_bits)
{
  __shared__ u64 keys[LINK_SMALL * LINK_SMALL], rowkey[LINK_SMALL], ekey[LINK_SMALL], eaux[LINK_SMALL];
  __shared__ u32 pairs[LINK_SMALL / 2];
  __shared__ int size[LINK_SMALL], nn[LINK_SMALL], n_new, bad_any;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, v = tid;
  if (tid == 0) bad_any = 0;
  if (tid < LINK_SMALL) { size[tid] = tid < ns ? 1 : 0; ekey[tid] = LINK_NONE; eaux[tid] = LINK_NONE; }
  __syncthreads ();
  int bad = 0;
  for (int x = tid; x < ns * ns; x += 256) {            // every cell beside its mirror, as linkage_small_kernel
    const int a = x / ns, b = x % ns;
    const u64 k = linkage_key (dist[x], dist[b * ns + a], a == b, metric, min_both, bad);
    if (linkage == TJAMD_AGGL_AVERAGE && k != LINK_NONE && k >= AGGL_KEY_MAX) bad |= 4;
    keys[a * LINK_SMALL + b] = k;
  }
  if (bad) atomicOr (&bad_any, bad);
  __syncthreads ();
  bad_bits = bad_any;
  if (bad_any) return -1;                               // (the whole workgroup)
  int n_links = 0, round = 0;                           // (the same in every thread)
  for (;; round++) {
    for (int a = wave; a < ns; a += 4) {                // (a) a wavefront per row, lane b
      u64 bk = LINK_NONE;
      int bb = lane;
      const int sa = size[a], sb = lane < ns ? size[lane] : 0;
      if (sa != 0 && sb != 0) {
        const u64 k = keys[a * LINK_SMALL + lane];
        if (k != LINK_NONE) bk = aggl_d (k, sa, sb, linkage);
      }
      wave_min_key_b (bk, bb);
      if (lane == 0) { rowkey[a] = bk; nn[a] = bk != LINK_NONE ? bb : -1; }
    }
    if (tid == 0) n_new = 0;
    __syncthreads ();
    if (v < ns && nn[v] > v && nn[nn[v]] == v) {        // (b) the mutual pairs, from their smaller ends
      const int at = atomicAdd (&n_new, 1), w = nn[v];
      pairs[at] = (u32) v << 12 | (u32) w;
      ekey[n_links + at] = rowkey[v]; eaux[n_links + at] = (u64) round << 24 | (u64) v << 12 | (u64) w;
    }
    __syncthreads ();
    const int n = n_new;
    if (n == 0) break;                                  // (the whole workgroup) no live cluster has an edge
    for (int x = tid; x < n * LINK_SMALL; x += 256) {   // (c) rows, then columns
      const int X = (int) (pairs[x >> 6] >> 12), Y = (int) (pairs[x >> 6] & 4095u), col = x & 63;
      if (col < ns) keys[X * LINK_SMALL + col] = aggl_f (keys[X * LINK_SMALL + col], keys[Y * LINK_SMALL + col], linkage);
    }
    __syncthreads ();
    for (int x = tid; x < n * LINK_SMALL; x += 256) {
      const int P = (int) (pairs[x >> 6] >> 12), Q = (int) (pairs[x >> 6] & 4095u), row = x & 63;
      if (row < ns) keys[row * LINK_SMALL + P] = aggl_f (keys[row * LINK_SMALL + P], keys[row * LINK_SMALL + Q], linkage);
    }
    if (tid < n) { const int X = (int) (pairs[tid] >> 12), Y = (int) (pairs[tid] & 4095u); size[X] += size[Y]; size[Y] = 0; }
    n_links += n;
    __syncthreads ();
  }
  lds_bitonic_sort<256> (ekey, eaux, LINK_SMALL);       // all 64 places, the empty ones last
  if (tid < n_links) mine = Link {(int) (eaux[tid] >> 12 & 4095u), (int) (eaux[tid] & 4095u), (long long) ekey[tid]};
  rounds = round;
  return n_links;
}

__global__ __launch_bounds__ (256)
void aggl_small_kernel (const SampleDistance *__restrict__ dist, int ns, int metric, int min_both, int linkage, Link *__restrict__ out, int *__restrict__ flags)
{
  const int tid = threadIdx.x;
  Link mine;
  int rounds, bad;
  const int n_links = aggl_small_body (dist, ns, metric, min_both, linkage, mine, rounds, bad);
  if (n_links < 0) { if (tid == 0) flags[0] = bad; return; }   // (the whole workgroup; nothing of the caller's is written)
  if (tid < n_links) out[tid] = mine;
  if (tid == 0) { flags[1] = 1; flags[2] = n_links; flags[3] = rounds; }
}

extern "C" long tjamd_sample_agglomerate (tjamd_counter *c, const tjamd_sample_distance *d_dist, int n_samples, int metric, int min_both, int linkage, tjamd_link *d_links,
                                          int *h_n_rounds)
{
  static const char *fn = "tjamd_sample_agglomerate";
  int rc = link_check_args (fn, c, d_dist, n_samples, metric, min_both, d_links);
  if (rc) return -rc;
  if (linkage != TJAMD_AGGL_COMPLETE && linkage != TJAMD_AGGL_AVERAGE) return -set_err (TJAMD_ERR_ARG, "%s: linkage %d outside 1..2", fn, linkage);
  Stage st (c, T_SAMPLE_AGGLOMERATE);                   // (a refused call leaves no timing behind)
  if (const int bad = st.enter (fn, "the tree is built")) return -bad;
  if (n_samples == 1) {                                 // one sample: no pair, no kernel
    rc = read_back (c, fn, nullptr, nullptr, 0);
    if (rc) return -rc;
    if (h_n_rounds) *h_n_rounds = 0;
    return 0;
  }
  const LinkShape shape (n_samples);
  const int ld = shape.ld, P = shape.P;
  const bool small = n_samples <= LINK_SMALL && c->link_small;   // one workgroup, one launch
  ScratchCut cut;
  int *flags, *size, *comp; LinkRowBest *rowbest; AgglEdge *edges; u32 *pairs; u64 *keys;
  cut.take (size, small ? 0 : (size_t) ld + 64); cut.take (comp, small ? 0 : (size_t) ld + 64); cut.take (rowbest, small ? 0 : (size_t) n_samples);
  cut.take (edges, small ? 0 : (size_t) n_samples); cut.take (pairs, small ? 0 : (size_t) n_samples); cut.take (keys, small ? 0 : (size_t) n_samples * ld);
  rc = commit_with_flags (cut, c, fn, flags);
  if (rc) return -rc;
  u32 h_flags[4] = {0, 0, 0, 0};
  st.begin ();
  if (small) {
    hipLaunchKernelGGL (aggl_small_kernel, dim3 (1), dim3 (256), 0, c->stream, (const SampleDistance *) d_dist, n_samples, metric, min_both, linkage, (Link *) d_links, flags);
    st.end ();
    rc = read_back (c, fn, flags, h_flags, 4);
    if (rc) return -rc;
  } else {
    const unsigned row_blocks = (unsigned) ((n_samples + 3) / 4);
    launch_linkage_keys (c, d_dist, n_samples, ld, metric, min_both, keys, comp, flags);   // (comp: N15's labels, not read here)
    hipLaunchKernelGGL (aggl_init_kernel, dim3 ((unsigned) std::min<long> (((long) n_samples * ld + 255) / 256, 4096)), dim3 (256), 0, c->stream, (const u64 *) keys, n_samples, ld,
                        linkage, size, flags);
    // a round that is not the last merges at least one pair: n_samples - 1 rounds at most.  A look at the flag words per batch.
    for (int queued = 0; queued < n_samples - 1 && !h_flags[0] && !h_flags[1]; ) {
      for (int r = 0; r < c->aggl_batch && queued < n_samples - 1; r++, queued++) {
        hipLaunchKernelGGL (aggl_rowmin_kernel, dim3 (row_blocks), dim3 (256), 0, c->stream, (const u64 *) keys, n_samples, ld, linkage, (const int *) size, rowbest, (const int *) flags);
        hipLaunchKernelGGL (aggl_pairs_kernel, dim3 (1), dim3 (1024), 0, c->stream, (const LinkRowBest *) rowbest, n_samples, size, edges, pairs, flags);
        hipLaunchKernelGGL (aggl_rows_kernel, dim3 ((unsigned) (n_samples / 2)), dim3 (256), 0, c->stream, keys, ld, linkage, (const u32 *) pairs, (const int *) flags);
        hipLaunchKernelGGL (aggl_cols_kernel, dim3 (row_blocks), dim3 (256), 0, c->stream, keys, n_samples, ld, linkage, (const int *) size, (const u32 *) pairs, (const int *) flags);
      }
      hipLaunchKernelGGL (aggl_sort_kernel, dim3 (1), dim3 (1024), 0, c->stream, (const AgglEdge *) edges, P, (Link *) d_links, (const int *) flags);
      st.end ();                                        // (the last one recorded is the one that is read)
      rc = read_back (c, fn, flags, h_flags, 4);
      if (rc) return -rc;
    }
  }
  if (h_flags[0] & 1u) return -set_err (TJAMD_ERR_ARG, CELL_REFUSED, fn);
  if (h_flags[0] & 2u) return -set_err (TJAMD_ERR_ARG, MIRROR_REFUSED, fn);
  if (h_flags[0] & 4u) return -set_err (TJAMD_ERR_ARG, "%s: a key of 2^40 or more under TJAMD_AGGL_AVERAGE", fn);
  if (!h_flags[1]) return -set_err (TJAMD_ERR_STATE, "%s: the rounds did not end", fn);
  st.done ();
  if (h_n_rounds) *h_n_rounds = (int) h_flags[3];
  return (long) h_flags[2];
}
TJ_LAST_MS (tjamd_last_sample_agglomerate_ms, T_SAMPLE_AGGLOMERATE)

// ---- N19: bootstrap support for the clades of the sample tree ----------------------------------------------------------------
// The rules as built are in include/tatajuba_bootstrap.h.
// bootstrap_weights_kernel: a thread per draw, blockIdx.y the replicate; the counts meet in integer atomic adds behind a memset.
// sample_distances_weighted: N14's check pass (it leaves `lens`), a pass over the weights (a workgroup per replicate: none below
//   0, a sum below 2^31), N14's tiles with the replicates as a new dimension, N14's summing pass with a replicate per blockIdx.y.
//   A workgroup stages a chunk once (sdist_stage) and walks it for SDISTW_BATCH = 2 replicates, whose weights lie beside the
//   chunk in LDS; the batches lie in blockIdx.z.  Two because a replicate's sums are 80 registers a thread (16 each of n_both,
//   same and the 32-bit length sums, 32 of the 64-bit ones): two of them and the walk fit 256 registers, two wavefronts a SIMD.
//   Where a wavefront's lanes share a site (edges 32 and 64) the weights are read into scalars, and a site whose two weights
//   are 0 (one in seven of a bootstrap's) is skipped by a uniform branch.  A pair costs four instructions that both replicates
//   share (the AND of the called bits, a compare and a select for the equal calls, one v_sad_u32 for |La - Lb|) and four per
//   replicate: c * w (v_mul_u32_u24), its add into n_both, the weight where the calls are equal, and one v_mad_u32_u24 of
//   |La - Lb| * (c * w) into the 32-bit length sum.  The 24-bit
//   multiplies hold while the call's largest weight and largest length are below 2^24 and their product within 32 bits, which
//   the weights' check works out; the 32-bit length sums are flushed when the products since the last flush would pass
//   2^32 - 1, and at a chunk's end.  A call beyond that is served by a second instance of the kernel (WIDE) with 32-bit
//   multiplies and a 64-bit product straight into the 64-bit sums.  Both instances are launched; each looks at what the check
//   left and one of them returns at once, so the host need not look in between.
// clade_support_kernel: a workgroup per replicate.  The replicate's order becomes pos[sample] in LDS, the base order
//   q[p] = pos[order[p]], the replicate's nodes a hash set of (first, size) in LDS (8192 places for 4095 nodes at most); a
//   wavefront per base node takes the minimum and maximum of q over the node's interval, and lane 0 asks the set for (minimum,
//   size) where the span is size.  The counts meet in scratch; a second kernel copies them out while no flag is up.

#define SDISTW_BATCH 2                                  // replicates a workgroup serves per staged chunk

// The replicates' arguments of N19 to N21, each where its entry's order of refusals has it: 0, or the code with its message set.
static int replicates_arg (const char *fn, int n) { return n < 1 || n > 4096 ? set_err (TJAMD_ERR_ARG, "%s: n_replicates %d outside 1..4096", fn, n) : 0; }
static int weights_count_arg (const char *fn, int n_replicates, long n_sites)
{
  return n_sites * (long) n_replicates >= (1l << 31) ? set_err (TJAMD_ERR_ARG, "%s: %d replicates x %ld sites: 2^31 weights or more", fn, n_replicates, n_sites) : 0;
}
// every replicate's count of nodes within 0..n_samples - 1, and the nodes' buffer where one has any; the counts are added to *total (may be null)
static int rep_nodes_args (const char *fn, const int *h_rep_n_nodes, int n_replicates, int n_samples, const tjamd_tree_node *d_rep_nodes, long *total)
{
  for (int r = 0; r < n_replicates; r++) {
    if (h_rep_n_nodes[r] < 0 || h_rep_n_nodes[r] > n_samples - 1)
      return set_err (TJAMD_ERR_ARG, "%s: replicate %d has %d nodes, outside 0..n_samples - 1 = %d", fn, r, h_rep_n_nodes[r], n_samples - 1);
    if (h_rep_n_nodes[r] > 0 && !d_rep_nodes) return set_err (TJAMD_ERR_ARG, "%s: null d_rep_nodes", fn);
    if (total) *total += h_rep_n_nodes[r];             // (a refused call does not read it)
  }
  return 0;
}

__device__ __forceinline__ u64 boot_mix (u64 z)
{
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31;
  return z;
}

__global__ __launch_bounds__ (256)
void bootstrap_weights_kernel (long n_sites, u64 seed, int *__restrict__ weights)
{
  const u64 base = boot_mix (seed + 0x9E3779B97F4A7C15ull * (u64) (blockIdx.y + 1));
  int *const mine = weights + blockIdx.y * n_sites;
  for (long j = blockIdx.x * 256l + threadIdx.x; j < n_sites; j += gridDim.x * 256l) {
    const u64 h = boot_mix (base + (u64) j);
    atomicAdd (mine + (long) (((h >> 32) * (u64) n_sites) >> 32), 1);   // ((h >> 32) < 2^32: the site is below n_sites)
  }
}

extern "C" long tjamd_bootstrap_weights (tjamd_counter *c, long n_sites, int n_replicates, unsigned long long seed, int *d_weights)
{
  static const char *fn = "tjamd_bootstrap_weights";
  if (!c) return -set_err (TJAMD_ERR_ARG, "%s: null counter", fn);
  if (!d_weights) return -set_err (TJAMD_ERR_ARG, "%s: null d_weights", fn);
  if (n_sites < 1 || n_sites >= (1l << 31)) return -set_err (TJAMD_ERR_ARG, "%s: n_sites %ld outside 1..2^31 - 1", fn, n_sites);
  if (const int bad = replicates_arg (fn, n_replicates)) return -bad;
  if (const int bad = weights_count_arg (fn, n_replicates, n_sites)) return -bad;
  Stage st (c, T_BOOTSTRAP_WEIGHTS);
  if (const int bad = st.enter (fn, "the weights are drawn")) return -bad;
  st.begin ();
  if (hipMemsetAsync (d_weights, 0, (size_t) (n_sites * n_replicates) * sizeof (int), c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: memset failed", fn);
  const long per_rep = std::max (1l, 8l * c->n_cu / n_replicates);
  hipLaunchKernelGGL (bootstrap_weights_kernel, dim3 ((unsigned) std::min ((n_sites + 255) / 256, per_rep), (unsigned) n_replicates), dim3 (256), 0, c->stream,
                      n_sites, (u64) seed, d_weights);
  st.end ();
  const int rc = read_back (c, fn, nullptr, nullptr, 0);
  if (rc) return -rc;
  st.done ();
  return n_replicates;
}
TJ_LAST_MS (tjamd_last_bootstrap_weights_ms, T_BOOTSTRAP_WEIGHTS)

// err bits beyond N14's: 256 a weight below 0, 512 a replicate whose weights sum to 2^31 or more.  A workgroup per replicate; each
// also takes its share of the sites.  err[2] and err[3] become the largest weight and the largest length (1023 at least) of the
// call: where both are below 2^24 and their product within 32 bits the tiles multiply in 24 bits and sum in 32 between
// flushes; a call beyond that is served by the WIDE instance of the tile kernel.  Either instance is launched and looks.
__global__ __launch_bounds__ (256)
void sample_weights_check_kernel (const int *__restrict__ weights, const Site *__restrict__ sites, long n_sites, int *__restrict__ err)
{
  __shared__ u64 part[4];
  const int *const mine = weights + blockIdx.x * n_sites;
  u64 sum = 0ull;
  int bad = 0, w_max = 0, l_max = 1023;
  for (long i = threadIdx.x; i < n_sites; i += 256) {
    const int w = mine[i];
    if (w < 0) bad = 256; else sum += (u64) w;
    w_max = max (w_max, w);
  }
  for (long i = blockIdx.x * 256l + threadIdx.x; i < n_sites; i += gridDim.x * 256l) l_max = max (l_max, sites[i].ref_length);
  for (int o = 32; o; o >>= 1) { sum += shfl_xor64 (sum, o); w_max = max (w_max, __shfl_xor (w_max, o)); l_max = max (l_max, __shfl_xor (l_max, o)); }
  if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6] = sum; atomicMax (err + 2, w_max); atomicMax (err + 3, l_max); }
  __syncthreads ();
  if (threadIdx.x == 0 && part[0] + part[1] + part[2] + part[3] >= (1ull << 31)) bad |= 512;
  if (bad) atomicOr (err, bad);
}

// what the weights' check left: does the call need the WIDE instance?
__device__ __forceinline__ bool sdist_weights_wide (const int *err)
{
  const u32 w = (u32) ((volatile const int *) err)[2], l = (u32) ((volatile const int *) err)[3];
  return w >= (1u << 24) || l >= (1u << 24) || (u64) w * l > 0xffffffffull;
}

template <int E, bool WIDE>                             // the tile's edge in samples, as in sample_distances_kernel; WIDE: see the weights' check
__global__ __launch_bounds__ (256, E >= 32 ? 2 : 1)     // (edges 32 and 64, where the work is: two workgroups a CU, two wavefronts a SIMD, 256 registers)
void sample_distances_weighted_kernel (const int16_t *__restrict__ gt, const int *__restrict__ lens, const int *__restrict__ weights, long n_sites, int ns, int n_rep,
                                       int n_tiles, long per_slice, SampleDistance *__restrict__ partial, SampleDistance *__restrict__ out, const int *__restrict__ err)
{
  constexpr int CH = SDIST_CELLS / E, T = E / 4, Z = 256 / (T * T), NB = SDISTW_BATCH;
  constexpr bool UNIFORM = T * T >= 64;                 // a wavefront's lanes are one thread group: they share the site, and so its weights
  __shared__ __attribute__ ((aligned (16))) int lds[4 * SDIST_CELLS];
  __shared__ int wl[NB][CH];                            // the chunk's weights, a row per replicate of the batch; 0 beyond the sites and the replicates
  __shared__ int l_max[2];
  if (*(volatile const int *) err != 0 || sdist_weights_wide (err) != WIDE) return;
  int *const gA = lds, *const lA = lds + SDIST_CELLS, *const gB = lds + 2 * SDIST_CELLS, *const lB = lds + 3 * SDIST_CELLS;
  int ti, tj;
  sdist_tile_pair (blockIdx.x, n_tiles, ti, tj);
  const int a0 = ti * E, b0 = tj * E, rep0 = blockIdx.z * NB;
  const long s_begin = blockIdx.y * per_slice, s_end = min (n_sites, s_begin + per_slice);
  const int tid = threadIdx.x, tx = tid % T, ty = (tid / T) % T, z = tid / (T * T);
  int nb[NB][4][4], same[NB][4][4];                     // per replicate as in N14, weighted
  u32 ld32[NB][4][4];
  u64 ld[NB][4][4];
  #pragma unroll
  for (int k = 0; k < NB; k++)
    #pragma unroll
    for (int r = 0; r < 4; r++)
      #pragma unroll
      for (int q = 0; q < 4; q++) { nb[k][r][q] = 0; same[k][r][q] = 0; ld32[k][r][q] = 0u; ld[k][r][q] = 0ull; }
  auto flush = [&] {
    #pragma unroll
    for (int k = 0; k < NB; k++)
      #pragma unroll
      for (int r = 0; r < 4; r++)
        #pragma unroll
        for (int q = 0; q < 4; q++) { ld[k][r][q] += ld32[k][r][q]; ld32[k][r][q] = 0u; }
  };
  if (tid == 0) l_max[0] = 1023;
  __syncthreads ();
  int parity = 0;
  for (long c0 = s_begin; c0 < s_end; c0 += CH, parity ^= 1) {
    for (int x = tid; x < NB * CH; x += 256) {
      const int k = x / CH;
      const long site = c0 + x % CH;
      wl[k][x % CH] = site < s_end && rep0 + k < n_rep ? weights[(long) (rep0 + k) * n_sites + site] : 0;
    }
    sdist_stage<E> (gt, lens, ns, a0, b0, c0, s_end, tid, gA, lA, gB, lB, l_max + parity);
    __syncthreads ();
    if (tid == 0) l_max[parity ^ 1] = 1023;
    u32 lmax = (u32) l_max[parity];
    if constexpr (UNIFORM) lmax = (u32) __builtin_amdgcn_readfirstlane ((int) lmax);
    // A site adds w * |La - Lb| <= w * the chunk's largest length to a pair's 32-bit sum: `room` is what the sums can still take
    // since the last flush, counted with the larger of the site's weights.
    u32 room = 0xffffffffu;
    const int n_here = (int) min ((long) CH, s_end - c0);
    for (int i = z; i < n_here; i += Z) {
      u32 w[NB], wmax = 0u;
      #pragma unroll
      for (int k = 0; k < NB; k++) {
        w[k] = (u32) wl[k][i];
        if constexpr (UNIFORM) w[k] = (u32) __builtin_amdgcn_readfirstlane ((int) w[k]);
        wmax = max (wmax, w[k]);
      }
      if (wmax == 0u) continue;                         // no replicate of the batch drew the site
      const int4 ga = *(const int4 *) (gA + i * E + 4 * ty), la = *(const int4 *) (lA + i * E + 4 * ty);
      const int4 gb = *(const int4 *) (gB + i * E + 4 * tx), lb = *(const int4 *) (lB + i * E + 4 * tx);
      const int gav[4] = {ga.x, ga.y, ga.z, ga.w}, gbv[4] = {gb.x, gb.y, gb.z, gb.w};
      const u32 lav[4] = {(u32) la.x, (u32) la.y, (u32) la.z, (u32) la.w}, lbv[4] = {(u32) lb.x, (u32) lb.y, (u32) lb.z, (u32) lb.w};
      u32 ca[4], cb[4];                                 // 1 where the cell is called, once per cell
      #pragma unroll
      for (int r = 0; r < 4; r++) { ca[r] = ~(u32) gav[r] >> 31; cb[r] = ~(u32) gbv[r] >> 31; }
      if constexpr (!WIDE) {                            // (weights and lengths below 2^24, the product of the largest two within 32 bits: the weights' check saw to it)
        const u32 cost = wmax * lmax;
        if (cost > room) { flush (); room = 0xffffffffu; }
        room -= cost;
        #pragma unroll
        for (int r = 0; r < 4; r++)
          #pragma unroll
          for (int q = 0; q < 4; q++) {                 // (no branch: the sixteen pairs of both replicates stay one straight run of instructions)
            const u32 c = ca[r] & cb[q], e = gav[r] == gbv[q] ? 1u : 0u, d = __usad (lav[r], lbv[q], 0u);   // (a missing cell equals nothing in the other tile)
            #pragma unroll
            for (int k = 0; k < NB; k++) {
              const u32 cw = __umul24 (c, w[k]);
              nb[k][r][q] += (int) cw;
              same[k][r][q] += (int) __umul24 (e, w[k]);
              ld32[k][r][q] += __umul24 (d, cw);
            }
          }
      }
      else {                                            // exact in 64 bits, past the 32-bit sums
        #pragma unroll
        for (int r = 0; r < 4; r++)
          #pragma unroll
          for (int q = 0; q < 4; q++) {
            const u32 c = ca[r] & cb[q], e = gav[r] == gbv[q] ? 1u : 0u, d = __usad (lav[r], lbv[q], 0u);
            #pragma unroll
            for (int k = 0; k < NB; k++) {
              const u32 cw = c * w[k];
              nb[k][r][q] += (int) cw;
              same[k][r][q] += (int) (e * w[k]);
              ld[k][r][q] += (u64) d * (u64) cw;        // (both below 2^31)
            }
          }
      }
    }
    flush ();
    __syncthreads ();
  }
  // where the sites are split: [replicate][slice][tile pair][E * E], a replicate's slices as sample_distances_reduce_kernel reads them
  #pragma unroll
  for (int k = 0; k < NB; k++) {
    const int rep = rep0 + k;
    if (rep >= n_rep) break;                            // (the whole workgroup)
    SampleDistance *const mine = partial ? partial + (((long) rep * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (E * E) : nullptr;
    sdist_store_tile<E> (nb[k], same[k], ld[k], lds, mine, out + (long) rep * ns * ns, ns, a0, b0, ti != tj, tid);
    if (Z > 1) __syncthreads ();                        // (the next replicate's sums meet where this one's did)
  }
}

extern "C" long tjamd_sample_distances_weighted (tjamd_counter *c, const tjamd_site *d_sites, long n_sites, const tjamd_allele *d_alleles, long n_alleles,
                                                 const int16_t *d_genotype, int n_samples, tjamd_sample_distance *d_out, const int *d_weights, int n_replicates)
{
  static const char *fn = "tjamd_sample_distances_weighted";
  if (!c) return -set_err (TJAMD_ERR_ARG, "%s: null counter", fn);
  if (const int bad = sdist_check_args (fn, d_sites, n_sites, d_alleles, n_alleles, d_genotype, n_samples, d_out)) return -bad;
  if (n_sites > 0 && !d_weights) return -set_err (TJAMD_ERR_ARG, "%s: null d_weights", fn);
  if (const int bad = replicates_arg (fn, n_replicates)) return -bad;
  if (const int bad = weights_count_arg (fn, n_replicates, n_sites)) return -bad;
  Stage st (c, T_SAMPLE_DISTANCES_WEIGHTED);            // (a refused call leaves no timing behind)
  if (const int bad = st.enter (fn, "the distances are summed")) return -bad;
  if (n_sites == 0) return sdist_empty (c, fn, d_out, n_samples, n_replicates);
  // N14's decomposition with the batches of replicates as a third dimension of the grid: the workgroups aimed at count tile pairs
  // x batches x slices, and the sites are split only where tile pairs x batches leave room.  Scratch, where they are split: a tile per
  // workgroup and replicate, bounded by the workgroups aimed at (two slices of edge 64 on 1024 workgroups, 128 MB, is the most).
  const long n_batches = (n_replicates + SDISTW_BATCH - 1) / SDISTW_BATCH;
  const SdistShape s (c, n_sites, n_samples, n_batches);
  SdistScratch x; SampleDistance *const out = (SampleDistance *) d_out;
  if (const int bad = sdist_head (st, fn, s, d_sites, n_sites, d_alleles, n_alleles, d_genotype, n_samples, n_replicates, x)) return -bad;
  hipLaunchKernelGGL (sample_weights_check_kernel, dim3 ((unsigned) n_replicates), dim3 (256), 0, c->stream, d_weights, (const Site *) d_sites, n_sites, x.err);
  for_edge (s.E, [&] (auto e) {                         // (one of the two walks the tiles, the other returns at once: the host does not look in between)
    constexpr int E = decltype (e)::value;
    for (int wd = 0; wd < 2; wd++)
      hipLaunchKernelGGL ((wd == 0 ? sample_distances_weighted_kernel<E, false> : sample_distances_weighted_kernel<E, true>), dim3 ((unsigned) s.n_pairs, (unsigned) s.n_slices, (unsigned) n_batches),
                          dim3 (256), 0, c->stream, d_genotype, (const int *) x.lens, d_weights, n_sites, n_samples, n_replicates, s.n_tiles, s.per_slice, x.partial, out, (const int *) x.err);
  });
  u32 h_err = 0;
  if (const int bad = sdist_tail (st, fn, s, x, n_samples, n_replicates, out, n_alleles, h_err)) return -bad;
  if (h_err & 256u) return -set_err (TJAMD_ERR_ARG, "%s: a weight is below 0", fn);
  if (h_err & 512u) return -set_err (TJAMD_ERR_ARG, "%s: the weights of a replicate sum to 2^31 or more", fn);
  st.done ();
  return n_sites;
}
TJ_LAST_MS (tjamd_last_sample_distances_weighted_ms, T_SAMPLE_DISTANCES_WEIGHTED)

#define CSUP_PLACES 8192                                // places of the set of a replicate's nodes: twice the most it can hold
__device__ __forceinline__ u32 csup_place (u32 key) { return (key * 0x9E3779B1u) >> 19; }   // (the top 13 bits)

// a permutation check's step over a cleared bitmap in LDS: raises the bit of s (in range: the caller saw to it) and says whether it
// was up.  ns positions on ns samples: one sample left out is one sample twice
__device__ __forceinline__ bool seen_twice (u32 *seen, int s) { return (atomicOr (&seen[s >> 5], 1u << (s & 31)) >> (s & 31)) & 1u; }

// flags[0] bits: 1 an order that is not a permutation, 2 a node outside the samples or of size < 2
__global__ __launch_bounds__ (1024)
void clade_support_kernel (const TreeNode *__restrict__ nodes, int n_nodes, const int *__restrict__ order, int ns, const TreeNode *__restrict__ rep_nodes,
                           const int *__restrict__ rep_order, const int *__restrict__ rep_n_nodes, int *__restrict__ cnt, int *__restrict__ flags)
{
  __shared__ u32 seen[CLD_MAX / 32];
  __shared__ unsigned short pos[CLD_MAX], qp[CLD_MAX];  // a sample's position in the replicate's order; the same, by position in the base order
  __shared__ u32 places[CSUP_PLACES];                   // first << 13 | size of a replicate's node (size >= 2: never 0), or 0
  const int tid = threadIdx.x, lane = tid & 63, rep = blockIdx.x;
  const int *const ro = rep_order + (long) rep * ns;
  const TreeNode *const rn = rep_nodes + (long) rep * (ns - 1);
  const int n_rn = rep_n_nodes[rep];                    // (0 .. ns - 1: the entry checked it)
  int bad = 0;
  for (int x = tid; x < CLD_MAX / 32; x += 1024) seen[x] = 0u;
  for (int x = tid; x < CSUP_PLACES; x += 1024) places[x] = 0u;
  for (int x = tid; x < CLD_MAX; x += 1024) pos[x] = 0;
  __syncthreads ();
  for (int p = tid; p < ns; p += 1024) {
    const int s = ro[p];
    if (s < 0 || s >= ns) { bad |= 1; continue; }
    if (seen_twice (seen, s)) bad |= 1;
    pos[s] = (unsigned short) p;
  }
  for (int k = tid; k < n_rn; k += 1024) {
    const TreeNode nd = rn[k];
    if (!tree_node_ok (nd, ns)) { bad |= 2; continue; }
    const u32 key = (u32) nd.first << 13 | (u32) nd.size;
    for (u32 at = csup_place (key); ; at = (at + 1) & (CSUP_PLACES - 1)) {   // (fewer nodes than half the places: a free one comes)
      const u32 old = atomicCAS (&places[at], 0u, key);
      if (old == 0u || old == key) break;               // (an equal node is in the set once)
    }
  }
  __syncthreads ();
  for (int x = tid; x < CLD_MAX / 32; x += 1024) seen[x] = 0u;
  __syncthreads ();
  for (int p = tid; p < ns; p += 1024) {
    const int s = order[p];
    if (s < 0 || s >= ns) { bad |= 1; qp[p] = 0; continue; }
    if (seen_twice (seen, s)) bad |= 1;
    qp[p] = pos[s];
  }
  __syncthreads ();
  for (int j = tid >> 6; j < n_nodes; j += 16) {        // a wavefront per node of the base
    const TreeNode nd = nodes[j];
    if (!tree_node_ok (nd, ns)) { bad |= 2; continue; }
    int lo = CLD_MAX, hi = -1;
    for (int p = nd.first + lane; p < nd.first + nd.size; p += 64) { const int v = qp[p]; lo = min (lo, v); hi = max (hi, v); }
    for (int o = 32; o; o >>= 1) { lo = min (lo, __shfl_xor (lo, o)); hi = max (hi, __shfl_xor (hi, o)); }
    if (lane == 0 && hi - lo + 1 == nd.size) {          // the members lie side by side in the replicate's order: is that interval a node there?
      const u32 key = (u32) lo << 13 | (u32) nd.size;
      for (u32 at = csup_place (key); ; at = (at + 1) & (CSUP_PLACES - 1)) {
        const u32 v = places[at];
        if (v == key) { atomicAdd (cnt + j, 1); break; }
        if (v == 0u) break;
      }
    }
  }
  if (bad) atomicOr (flags, bad);
}

__global__ __launch_bounds__ (256)
void clade_support_store_kernel (const int *__restrict__ cnt, int n_nodes, int *__restrict__ support, const int *__restrict__ flags)
{
  if (*(volatile const int *) flags != 0) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < n_nodes) support[j] = cnt[j];
}

extern "C" long tjamd_clade_support (tjamd_counter *c, const tjamd_tree_node *d_nodes, int n_nodes, const int *d_order, int n_samples, const tjamd_tree_node *d_rep_nodes,
                                     const int *d_rep_order, const int *h_rep_n_nodes, int n_replicates, int *d_support)
{
  static const char *fn = "tjamd_clade_support";
  if (!c) return -set_err (TJAMD_ERR_ARG, "%s: null counter", fn);
  if (n_samples < 1 || n_samples > CLD_MAX) return -set_err (TJAMD_ERR_ARG, "%s: n_samples %d outside 1..4096", fn, n_samples);
  if (n_nodes < 0 || n_nodes > CLD_MAX) return -set_err (TJAMD_ERR_ARG, "%s: n_nodes %d outside 0..4096", fn, n_nodes);
  if (const int bad = replicates_arg (fn, n_replicates)) return -bad;
  if (!d_order || !d_rep_order) return -set_err (TJAMD_ERR_ARG, "%s: null d_order or d_rep_order", fn);
  if (!h_rep_n_nodes) return -set_err (TJAMD_ERR_ARG, "%s: null h_rep_n_nodes", fn);
  if (n_nodes > 0 && (!d_nodes || !d_support)) return -set_err (TJAMD_ERR_ARG, "%s: null d_nodes or d_support", fn);
  if (const int bad = rep_nodes_args (fn, h_rep_n_nodes, n_replicates, n_samples, d_rep_nodes, nullptr)) return -bad;
  Stage st (c, T_CLADE_SUPPORT);                        // (a refused call leaves no timing behind)
  if (const int bad = st.enter (fn, "the clades are compared")) return -bad;
  int rc;
  if (n_nodes == 0) {                                   // no clade to ask about: no kernel
    rc = read_back (c, fn, nullptr, nullptr, 0);
    return rc ? -rc : 0;
  }
  ScratchCut cut;
  int *flags, *cnt, *rep_n;
  cut.take (cnt, (size_t) n_nodes); cut.take (rep_n, (size_t) n_replicates);
  rc = commit_with_flags (cut, c, fn, flags);
  if (rc) return -rc;
  if (hipMemsetAsync (cnt, 0, (size_t) n_nodes * sizeof (int), c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: memset failed", fn);
  if (hipMemcpyAsync (rep_n, h_rep_n_nodes, (size_t) n_replicates * sizeof (int), hipMemcpyHostToDevice, c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: copy failed", fn);
  st.begin ();
  hipLaunchKernelGGL (clade_support_kernel, dim3 ((unsigned) n_replicates), dim3 (1024), 0, c->stream, (const TreeNode *) d_nodes, n_nodes, d_order, n_samples,
                      (const TreeNode *) d_rep_nodes, d_rep_order, (const int *) rep_n, cnt, flags);
  hipLaunchKernelGGL (clade_support_store_kernel, dim3 ((unsigned) ((n_nodes + 255) / 256)), dim3 (256), 0, c->stream, (const int *) cnt, n_nodes, d_support, (const int *) flags);
  st.end ();
  u32 h_flags[1] = {0};
  rc = read_back (c, fn, flags, h_flags, 1);
  if (rc) return -rc;
  if (h_flags[0] & 1u) return -set_err (TJAMD_ERR_ARG, "%s: d_order or a replicate's order is not a permutation of 0 .. n_samples - 1", fn);
  if (h_flags[0] & 2u) return -set_err (TJAMD_ERR_ARG, "%s: a node has size < 2, first < 0 or first + size above n_samples %d", fn, n_samples);
  st.done ();
  return n_nodes;
}
TJ_LAST_MS (tjamd_last_clade_support_ms, T_CLADE_SUPPORT)

// ---- N20: the trees of all bootstrap replicates in one call -------------------------------------------------------------------
// The rule as built is in include/tatajuba_replicate_trees.h: per replicate the bytes of N15's or N18's builder and of N17's
// tree.  The bodies of their kernels run here with the replicate taken from the grid (blockIdx.y; blockIdx.z in the key pass),
// every array of a call strided by the replicate; nothing of those bodies is restated.
//   0. rep_check_kernel, all replicates of the call at once: N15's tiles without the stores, and N18's bound under AVERAGE.
//      A replicate's error bits go to its flag words, their OR to the call's error word.  It is complete before any other
//      kernel of the call starts, every other kernel returns at once while the call's word is up, and so a refused call
//      writes nothing of the caller's, whatever the group of the bad replicate (why not staging).
//   Up to 64 samples, rep_trees_small_kernel: a workgroup per replicate; linkage_small_body or aggl_small_body leave the sorted
//      links in registers, a link a thread; they go to LDS, and tree_small builds N17's nodes and the leaf order there.
//   Beyond, per group of replicates: rep_keys_kernel, the rounds (N15: ceil (log2 n_samples) times rowmin and merge, no look at
//      the device; N18: batches of aggl_batch rounds of four kernels and the sort, one look per batch for the whole group, until
//      every replicate of the group is done: a replicate that is done returns at once from every kernel), then rep_tree_kernel,
//      a workgroup per replicate with linkage_tree_body on the replicate's links in scratch.
// flag words of a replicate (8): [0] its error bits, [1] to [4] as N15 / N18 use them, [5] the tree's error word (0: the links
// are the builder's own), [6] its links are sorted (N18's sort runs behind every batch), [7] the call's error word as the sort
// kernel saw it (the host's one copy per batch brings it along).

#define REP_FLAGS 8

struct RepCut                                           // the scratch of a group: piece + replicate * stride
{
  u64 *keys; int *comp, *size; LinkRowBest *rowbest; LinkEdge *edges; u32 *pairs; Link *links; int *rflags; const int *flags;
  int ns, ld, ldc;                                      // ldc: the stride of comp and size (ld + 64 words at least, a multiple of 64)
  __device__ __forceinline__ u64 *keys_of (int g) const { return keys + (long) g * ns * ld; }
  __device__ __forceinline__ int *comp_of (int g) const { return comp + (long) g * ldc; }
  __device__ __forceinline__ int *size_of (int g) const { return size + (long) g * ldc; }
  __device__ __forceinline__ LinkRowBest *rowbest_of (int g) const { return rowbest + (long) g * ns; }
  __device__ __forceinline__ LinkEdge *edges_of (int g) const { return edges + (long) g * ns; }
  __device__ __forceinline__ AgglEdge *aggl_edges_of (int g) const { return (AgglEdge *) edges + (long) g * ns; }
  __device__ __forceinline__ u32 *pairs_of (int g) const { return pairs + (long) g * ns; }
  __device__ __forceinline__ Link *links_of (int g) const { return links + (long) g * (ns - 1); }
  __device__ __forceinline__ int *flags_of (int g) const { return rflags + (long) g * REP_FLAGS; }
  __device__ __forceinline__ bool refused () const { return *(volatile const int *) flags != 0; }
};
static_assert (sizeof (LinkEdge) == sizeof (AgglEdge), "one stride for the edges of both builders");

__global__ __launch_bounds__ (256)
void rep_check_kernel (const SampleDistance *__restrict__ dist, int ns, int ld, int metric, int min_both, u64 key_max, int *__restrict__ rflags, int *__restrict__ flags)
{
  const int r = blockIdx.z;
  const int bad = linkage_keys_tile<false> (dist + (long) r * ns * ns, ns, ld, metric, min_both, key_max, nullptr);
  if (bad) { atomicOr (&rflags[(long) r * REP_FLAGS], bad); atomicOr (flags, bad); }
}

// N17's tree of at most 63 links on at most 64 samples, as linkage_tree_body builds it, by a workgroup of 256: the links in
// LDS, lane 0 walks them up and the nodes down, wavefront 0 lays the roots out (sample v in lane v).  The links are the
// builder's own: no check, and the walk is bounded by n_links < ns all the same.
__device__ __forceinline__ void tree_small (const Link *sl, int n_links, int ns, TreeNode *__restrict__ nodes, int *__restrict__ order)
{
  __shared__ int uf[LINK_SMALL], cnode[LINK_SMALL], nl[LINK_SMALL], nr[LINK_SMALL], nsz[LINK_SMALL], nfi[LINK_SMALL], ord[LINK_SMALL];
  const int tid = threadIdx.x;
  if (tid < ns) { uf[tid] = tid; cnode[tid] = -1 - tid; }
  __syncthreads ();
  if (tid == 0)
    for (int j = 0; j < n_links; j++) {
      int ra = sl[j].a, rb = sl[j].b;
      while (uf[ra] != ra) { const int up = uf[uf[ra]]; uf[ra] = up; ra = up; }
      while (uf[rb] != rb) { const int up = uf[uf[rb]]; uf[rb] = up; rb = up; }
      const int lo = min (ra, rb), hi = max (ra, rb), cl = cnode[lo], cr = cnode[hi];
      nl[j] = cl; nr[j] = cr; nsz[j] = (cl >= 0 ? nsz[cl] : 1) + (cr >= 0 ? nsz[cr] : 1);
      uf[hi] = lo; cnode[lo] = j;
    }
  __syncthreads ();
  if (tid < 64) {                                       // the roots in the order of their smallest member
    const bool root = tid < ns && uf[tid] == tid;
    const int cn = root ? cnode[tid] : -1, mine = !root ? 0 : cn >= 0 ? nsz[cn] : 1;
    const int incl = wave_inclusive_sum (mine, tid);
    if (root) { if (cn >= 0) nfi[cn] = incl - mine; else ord[incl - mine] = tid; }
  }
  __syncthreads ();
  if (tid == 0)
    for (int j = n_links - 1; j >= 0; j--) {            // a parent comes before its children
      const int f = nfi[j], l = nl[j], r = nr[j], fr = f + (l >= 0 ? nsz[l] : 1);
      if (l >= 0) nfi[l] = f; else ord[f] = -1 - l;
      if (r >= 0) nfi[r] = fr; else ord[fr] = -1 - r;
    }
  __syncthreads ();
  if (tid < n_links) nodes[tid] = TreeNode {nl[tid], nr[tid], nfi[tid], nsz[tid]};
  if (tid < ns) order[tid] = ord[tid];
}

template <bool AGGL>
__global__ __launch_bounds__ (256)
void rep_trees_small_kernel (const SampleDistance *__restrict__ dist, int ns, int metric, int min_both, int linkage, int n_rounds, Link *__restrict__ links_out,
                             TreeNode *__restrict__ nodes, int *__restrict__ order, int *__restrict__ rflags, const int *__restrict__ flags)
{
  __shared__ Link sl[LINK_SMALL];
  if (*(volatile const int *) flags != 0) return;       // (the whole workgroup) a replicate of the call is refused
  const int tid = threadIdx.x, r = blockIdx.x;
  const SampleDistance *d = dist + (long) r * ns * ns;
  Link mine = Link {0, 0, 0};
  int rounds = 0, bad = 0, n;
  if (AGGL) n = aggl_small_body (d, ns, metric, min_both, linkage, mine, rounds, bad);
  else n = linkage_small_body (d, ns, metric, min_both, n_rounds, mine, bad);
  if (n < 0) return;                                    // (the check pass has read every cell: not taken)
  if (tid < n) {
    sl[tid] = mine;
    if (links_out) links_out[(long) r * (ns - 1) + tid] = mine;
  }
  if (tid == 0) { rflags[(long) r * REP_FLAGS + 1] = 1; rflags[(long) r * REP_FLAGS + 2] = n; rflags[(long) r * REP_FLAGS + 3] = rounds; }
  __syncthreads ();
  tree_small (sl, n, ns, nodes + (long) r * (ns - 1), order + (long) r * ns);
}

__global__ __launch_bounds__ (256)
void rep_keys_kernel (RepCut A, const SampleDistance *__restrict__ dist, int metric, int min_both)
{
  if (A.refused ()) return;
  const int g = blockIdx.z, tid = threadIdx.x, b0 = blockIdx.x * LINK_TILE;
  if (blockIdx.y == 0 && tid < LINK_TILE && b0 + tid < A.ld) {   // every sample its own component, and a cluster of size 1 (the padding column: a retired cluster)
    A.comp_of (g)[b0 + tid] = b0 + tid;
    A.size_of (g)[b0 + tid] = b0 + tid < A.ns ? 1 : 0;
  }
  (void) linkage_keys_tile<true> (dist + (long) g * A.ns * A.ns, A.ns, A.ld, metric, min_both, LINK_NONE, A.keys_of (g));
}

__global__ __launch_bounds__ (256)
void rep_linkage_rowmin_kernel (RepCut A)
{
  const int g = blockIdx.y;
  if (A.refused ()) return;
  linkage_rowmin_body (A.keys_of (g), A.ns, A.ld, A.comp_of (g), A.rowbest_of (g), A.flags_of (g));
}

__global__ __launch_bounds__ (1024)
void rep_linkage_merge_kernel (RepCut A, int n_jump)
{
  const int g = blockIdx.y;
  if (A.refused ()) return;
  linkage_merge_body (A.rowbest_of (g), A.ns, n_jump, A.comp_of (g), A.edges_of (g), A.flags_of (g));
}

__global__ __launch_bounds__ (1024)
void rep_linkage_sort_kernel (RepCut A, int P)
{
  const int g = blockIdx.y;
  if (A.refused ()) return;
  linkage_sort_body (A.edges_of (g), P, A.links_of (g), A.flags_of (g));
}

__global__ __launch_bounds__ (256)
void rep_aggl_rowmin_kernel (RepCut A, int linkage)
{
  const int g = blockIdx.y;
  if (A.refused ()) return;
  aggl_rowmin_body (A.keys_of (g), A.ns, A.ld, linkage, A.size_of (g), A.rowbest_of (g), A.flags_of (g));
}

__global__ __launch_bounds__ (1024)
void rep_aggl_pairs_kernel (RepCut A)
{
  const int g = blockIdx.y;
  if (A.refused ()) return;
  aggl_pairs_body (A.rowbest_of (g), A.ns, A.size_of (g), A.aggl_edges_of (g), A.pairs_of (g), A.flags_of (g));
}

__global__ __launch_bounds__ (256)
void rep_aggl_rows_kernel (RepCut A, int linkage)
{
  const int g = blockIdx.y;
  if (A.refused ()) return;
  aggl_rows_body (A.keys_of (g), A.ld, linkage, A.pairs_of (g), A.flags_of (g));
}

__global__ __launch_bounds__ (256)
void rep_aggl_cols_kernel (RepCut A, int linkage)
{
  const int g = blockIdx.y;
  if (A.refused ()) return;
  aggl_cols_body (A.keys_of (g), A.ns, A.ld, linkage, A.size_of (g), A.pairs_of (g), A.flags_of (g));
}

__global__ __launch_bounds__ (1024)
void rep_aggl_sort_kernel (RepCut A, int P)
{
  const int g = blockIdx.y;
  int *const f = A.flags_of (g);
  const int refused = *(volatile const int *) A.flags;
  if (refused) { if (threadIdx.x == 0) f[7] = refused; return; }   // (what the host reads per batch)
  if (f[6]) return;                                     // sorted behind an earlier batch
  const bool done = ((volatile const int *) f)[1] != 0; // (the whole workgroup reads one word that no kernel of this launch writes)
  aggl_sort_body (A.aggl_edges_of (g), P, A.links_of (g), f);
  if (done && threadIdx.x == 0) f[6] = 1;
}

__global__ __launch_bounds__ (1024)
void rep_tree_kernel (RepCut A, Link *__restrict__ links_out, TreeNode *__restrict__ nodes, int *__restrict__ order)
{
  const int g = blockIdx.x;
  if (A.refused ()) return;
  int *const f = A.flags_of (g);
  const int n_links = f[2], ns = A.ns;                  // (0 .. ns - 1: the builders append fewer than ns links)
  const Link *links = A.links_of (g);
  if (links_out)
    for (int j = threadIdx.x; j < n_links; j += 1024) links_out[(long) g * (ns - 1) + j] = links[j];
  linkage_tree_body (links, n_links, ns, nodes + (long) g * (ns - 1), order + (long) g * ns, f + 5);
}

extern "C" long tjamd_replicate_trees (tjamd_counter *c, const tjamd_sample_distance *d_dist, int n_samples, int n_replicates, int metric, int min_both, int linkage,
                                       tjamd_link *d_rep_links, tjamd_tree_node *d_rep_nodes, int *d_rep_order, int *h_rep_n_nodes, int *h_rep_n_rounds)
{
  static const char *fn = "tjamd_replicate_trees";
  if (!c) return -set_err (TJAMD_ERR_ARG, "%s: null counter", fn);
  if (!d_dist) return -set_err (TJAMD_ERR_ARG, "%s: null d_dist", fn);
  if (!d_rep_order) return -set_err (TJAMD_ERR_ARG, "%s: null d_rep_order", fn);
  if (!h_rep_n_nodes) return -set_err (TJAMD_ERR_ARG, "%s: null h_rep_n_nodes", fn);
  if (!d_rep_nodes && n_samples > 1) return -set_err (TJAMD_ERR_ARG, "%s: null d_rep_nodes", fn);
  if (n_samples < 1 || n_samples > LINK_MAX) return -set_err (TJAMD_ERR_ARG, "%s: n_samples %d outside 1..4096", fn, n_samples);
  if (const int bad = replicates_arg (fn, n_replicates)) return -bad;
  if (metric < TJAMD_LINK_DIFFER || metric > TJAMD_LINK_DIFFER_RATE) return -set_err (TJAMD_ERR_ARG, "%s: metric %d outside 0..2", fn, metric);
  if (min_both < 1) return -set_err (TJAMD_ERR_ARG, "%s: min_both %d below 1", fn, min_both);
  if (linkage != TJAMD_TREE_SINGLE && linkage != TJAMD_AGGL_COMPLETE && linkage != TJAMD_AGGL_AVERAGE) return -set_err (TJAMD_ERR_ARG, "%s: linkage %d outside 0..2", fn, linkage);
  Stage st (c, T_REPLICATE_TREES);                      // (a refused call leaves no timing behind)
  if (const int bad = st.enter (fn, "the trees are built")) return -bad;
  const int ns = n_samples, R = n_replicates;
  int rc;
  if (ns == 1) {                                        // one sample: no pair, no kernel; every order is the sample 0
    if (hipMemsetAsync (d_rep_order, 0, (size_t) R * sizeof (int), c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: memset failed", fn);
    rc = read_back (c, fn, nullptr, nullptr, 0);
    if (rc) return -rc;
    for (int r = 0; r < R; r++) { h_rep_n_nodes[r] = 0; if (h_rep_n_rounds) h_rep_n_rounds[r] = 0; }
    return R;
  }
  const LinkShape shape (ns);
  const int ld = shape.ld, P = shape.P, ldc = (ld + 64 + 63) & ~63;
  int n_rounds = 0;
  while ((1 << n_rounds) < ns) n_rounds++;              // N15: every round at least halves the components that still have an edge
  const bool aggl = linkage != TJAMD_TREE_SINGLE, small = ns <= LINK_SMALL && c->link_small;
  // the replicates of a group: what REP_SCRATCH_CAP holds of one replicate's pieces (each rounded up as the cut rounds the group's)
  const size_t per = small ? 0 : (size_t) ns * ld * 8 + 2 * (size_t) ldc * 4 + 2 * (size_t) ns * 16 + (size_t) ns * 4 + (size_t) (ns - 1) * 16;
  const size_t REP_SCRATCH_CAP = (size_t) 1 << 30;
  const int G = c->trees_group ? std::min (R, c->trees_group) : small ? R : (int) std::max<size_t> (1, std::min<size_t> ((size_t) R, REP_SCRATCH_CAP / per));
  const size_t Gs = small ? 0 : (size_t) G;
  ScratchCut cut;
  RepCut A;
  int *flags;
  cut.take (A.comp, Gs * ldc); cut.take (A.size, Gs * ldc); cut.take (A.rowbest, Gs * ns); cut.take (A.edges, Gs * ns); cut.take (A.pairs, Gs * ns);
  cut.take (A.links, Gs * (ns - 1)); cut.take (A.keys, Gs * ns * ld); cut.take (A.rflags, (size_t) R * REP_FLAGS);
  rc = commit_with_flags (cut, c, fn, flags);
  if (rc) return -rc;
  int *const rflags = A.rflags;                         // (of replicate 0; A.rflags moves with the group)
  A.flags = flags; A.ns = ns; A.ld = ld; A.ldc = ldc;
  if (hipMemsetAsync (rflags, 0, (size_t) R * REP_FLAGS * sizeof (int), c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: memset failed", fn);
  std::vector<int> h_rf ((size_t) R * REP_FLAGS, 0);
  const SampleDistance *dist = (const SampleDistance *) d_dist;
  const unsigned tiles_x = (unsigned) ((ld + LINK_TILE - 1) / LINK_TILE), tiles_y = (unsigned) ((ns + LINK_TILE - 1) / LINK_TILE), row_blocks = (unsigned) ((ns + 3) / 4);
  st.begin ();
  hipLaunchKernelGGL (rep_check_kernel, dim3 (tiles_x, tiles_y, (unsigned) R), dim3 (256), 0, c->stream, dist, ns, ld, metric, min_both,
                      linkage == TJAMD_AGGL_AVERAGE ? AGGL_KEY_MAX : LINK_NONE, rflags, flags);
  bool refused = false;
  for (int r0 = 0; r0 < R && !refused; r0 += G) {
    const unsigned g = (unsigned) std::min (G, R - r0);
    const SampleDistance *gdist = dist + (size_t) r0 * ns * ns;
    Link *glinks = d_rep_links ? (Link *) d_rep_links + (size_t) r0 * (ns - 1) : nullptr;
    TreeNode *gnodes = (TreeNode *) d_rep_nodes + (size_t) r0 * (ns - 1);
    int *gorder = d_rep_order + (size_t) r0 * ns;
    A.rflags = rflags + (size_t) r0 * REP_FLAGS;
    if (small) {
      if (aggl) hipLaunchKernelGGL (rep_trees_small_kernel<true>, dim3 (g), dim3 (256), 0, c->stream, gdist, ns, metric, min_both, linkage, n_rounds, glinks, gnodes, gorder, A.rflags, (const int *) flags);
      else hipLaunchKernelGGL (rep_trees_small_kernel<false>, dim3 (g), dim3 (256), 0, c->stream, gdist, ns, metric, min_both, linkage, n_rounds, glinks, gnodes, gorder, A.rflags, (const int *) flags);
      continue;
    }
    hipLaunchKernelGGL (rep_keys_kernel, dim3 (tiles_x, tiles_y, g), dim3 (256), 0, c->stream, A, gdist, metric, min_both);
    if (!aggl) {
      for (int r = 0; r < n_rounds; r++) {
        hipLaunchKernelGGL (rep_linkage_rowmin_kernel, dim3 (row_blocks, g), dim3 (256), 0, c->stream, A);
        hipLaunchKernelGGL (rep_linkage_merge_kernel, dim3 (1, g), dim3 (1024), 0, c->stream, A, n_rounds);
      }
      hipLaunchKernelGGL (rep_linkage_sort_kernel, dim3 (1, g), dim3 (1024), 0, c->stream, A, P);
    } else {
      // N18's batches: a look at the group's flag words per batch; the rounds enqueued are those of the group's slowest replicate
      bool over = false;
      for (int queued = 0; queued < ns - 1 && !over && !refused; ) {
        for (int r = 0; r < c->aggl_batch && queued < ns - 1; r++, queued++) {
          hipLaunchKernelGGL (rep_aggl_rowmin_kernel, dim3 (row_blocks, g), dim3 (256), 0, c->stream, A, linkage);
          hipLaunchKernelGGL (rep_aggl_pairs_kernel, dim3 (1, g), dim3 (1024), 0, c->stream, A);
          hipLaunchKernelGGL (rep_aggl_rows_kernel, dim3 ((unsigned) (ns / 2), g), dim3 (256), 0, c->stream, A, linkage);
          hipLaunchKernelGGL (rep_aggl_cols_kernel, dim3 (row_blocks, g), dim3 (256), 0, c->stream, A, linkage);
        }
        hipLaunchKernelGGL (rep_aggl_sort_kernel, dim3 (1, g), dim3 (1024), 0, c->stream, A, P);
        st.end ();
        int *h = h_rf.data () + (size_t) r0 * REP_FLAGS;
        rc = read_back (c, fn, A.rflags, h, (size_t) g * REP_FLAGS);
        if (rc) return -rc;
        over = true;
        for (unsigned k = 0; k < g; k++) { if (h[k * REP_FLAGS + 7]) refused = true; if (!h[k * REP_FLAGS + 1]) over = false; }
      }
      if (refused) break;
      if (!over) return -set_err (TJAMD_ERR_STATE, "%s: the rounds did not end", fn);
    }
    hipLaunchKernelGGL (rep_tree_kernel, dim3 (g), dim3 (1024), 0, c->stream, A, glinks, gnodes, gorder);
  }
  st.end ();
  rc = read_back (c, fn, rflags, h_rf.data (), (size_t) R * REP_FLAGS);
  if (rc) return -rc;
  for (int r = 0; r < R; r++) {                         // the smallest refused replicate, its first broken rule in N15's / N18's order
    const int bad = h_rf[(size_t) r * REP_FLAGS];
    if (!bad) continue;
    char text[256];
    snprintf (text, sizeof text, bad & 1 ? CELL_REFUSED : bad & 2 ? MIRROR_REFUSED : "%s: a key of 2^40 or more under TJAMD_AGGL_AVERAGE", fn);
    return -set_err (TJAMD_ERR_ARG, "%s (replicate %d)", text, r);
  }
  for (int r = 0; r < R; r++)
    if (h_rf[(size_t) r * REP_FLAGS + 5]) return -set_err (TJAMD_ERR_STATE, "%s: the links of replicate %d are no forest", fn, r);
  st.done ();
  for (int r = 0; r < R; r++) {
    h_rep_n_nodes[r] = h_rf[(size_t) r * REP_FLAGS + 2];
    if (h_rep_n_rounds) h_rep_n_rounds[r] = aggl ? h_rf[(size_t) r * REP_FLAGS + 3] : 0;
  }
  return R;
}
TJ_LAST_MS (tjamd_last_replicate_trees_ms, T_REPLICATE_TREES)

// ---- N21: the majority-rule consensus tree of the bootstrap replicates ----------------------------------------------------------
// The rule as built is in include/tatajuba_consensus.h.  A clade is a record: its index g = rep_off[r] + k among all nodes of
// the call, and a key (size << 51 | the low bits of a hash sum over its members).  Equal sets have equal keys; equal keys are
// told apart by comparing sets, so nothing rests on the hash.
//   1. cons_records_kernel, a workgroup per replicate: the permutation, the nodes and the crossing check (far[p]: the furthest
//      end of the nodes that start at p; a node crosses another exactly when a node that starts inside it ends behind it), the
//      positions of the samples to scratch, the prefix sums of the hashes in LDS, a record per node.  Error bits go to the
//      replicate's word and to the call's; every later kernel returns at once while the call's word is up.
//   2. kv_sort on all 64 bits; cons_heads_kernel and a scan number the runs of equal keys.
//   3. rounds: cons_lead_kernel takes the first unsettled record of every run as its leader (an integer minimum), and
//      cons_compare_kernel, a wavefront per unsettled record, settles the leader itself and every record whose set is the
//      leader's.  The host reads one word per round and goes on while a record is unsettled.
//   4. cons_count_kernel: a record counts for its class unless an earlier record of its run has its class and its replicate
//      (those lie next to each other: the sort is stable and the records were emitted replicate by replicate).
//   5. cons_kept_kernel hands the counts out and lists the leaders of the kept classes; cons_info_kernel, a wavefront per kept
//      class, finds its smallest member; cons_order_kernel ranks them by (size, smallest member); cons_parent_kernel, a
//      wavefront per kept class, finds the first larger class that holds its smallest member (laminar: that class holds all of
//      it) and marks its members' smallest class; cons_layout_kernel lays nodes and samples out.
// flag words of the call: [0] error bits (1 order, 2 node, 4 crossing), [1] a record is unsettled after this round, [2] kept
// classes, [3] classes, [4] more kept classes than n_samples - 1 (cannot be: a laminar family).

#define CONS_KEY_BITS 51
#define CONS_SALT 0x5851F42D4C957F2Dull
#define CONS_NONE 0xFFFFu

struct ConsNode { int parent, count, first, size; };
struct ConsKept { int size, minm, count, rep, first, pad; };   // rep, first: where the class's leader lies
static_assert (sizeof (ConsNode) == sizeof (tjamd_consensus_node) && sizeof (ConsNode) == sizeof (TreeNode), "a consensus node is read as a tree node");
static_assert (offsetof (ConsNode, first) == offsetof (TreeNode, first) && offsetof (ConsNode, size) == offsetof (TreeNode, size), "first and size where tjamd_tree_node has them");

struct ConsIn                                           // the replicates of a call, as every kernel of it reads them
{
  const TreeNode *rep_nodes; const int *rep_order, *rep_n, *rep_off; const unsigned short *pos; int ns, R;
  __device__ __forceinline__ int rep_of (int g) const   // the replicate of record g: the last one that starts at or before it
  {
    int lo = 0, hi = R;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (rep_off[mid] <= g) lo = mid; else hi = mid; }
    return lo;
  }
  __device__ __forceinline__ TreeNode node_of (int g, int r) const { return rep_nodes[(long) r * (ns - 1) + (g - rep_off[r])]; }
  __device__ __forceinline__ const int *members_of (int r, int first) const { return rep_order + (long) r * ns + first; }
};

__global__ __launch_bounds__ (1024)
void cons_records_kernel (ConsIn A, u64 key_mask, unsigned short *__restrict__ pos_out, u64 *__restrict__ key, u32 *__restrict__ val, int *__restrict__ rbad, int *__restrict__ flags)
{
  __shared__ u32 seen[CLD_MAX / 32];
  __shared__ int far[CLD_MAX];                          // the furthest end of the nodes that start at a position, or 0
  __shared__ u64 pre[CLD_MAX + 1];                      // pre[p]: the wrapping sum of the hashes of the samples before position p
  __shared__ u64 wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x, ns = A.ns;
  const int *const ro = A.rep_order + (long) r * ns;
  const TreeNode *const rn = A.rep_nodes + (long) r * (ns - 1);
  const int n_rn = A.rep_n[r], off = A.rep_off[r];      // (0 .. ns - 1: the entry checked it)
  int bad = 0;
  for (int x = tid; x < CLD_MAX / 32; x += 1024) seen[x] = 0u;
  for (int x = tid; x < CLD_MAX; x += 1024) far[x] = 0;
  __syncthreads ();
  u64 run[4], total = 0;                                // four positions a thread
  #pragma unroll
  for (int q = 0; q < 4; q++) {
    const int p = tid * 4 + q;
    u64 h = 0;
    if (p < ns) {
      const int s = ro[p];
      if (s < 0 || s >= ns) bad |= 1;
      else {
        if (seen_twice (seen, s)) bad |= 1;
        pos_out[(long) r * ns + s] = (unsigned short) p;
        h = boot_mix (CONS_SALT + (u64) s);
      }
    }
    total += h; run[q] = total;
  }
  const u64 incl = wave_inclusive_sum (total, lane);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads ();
  u64 base = incl - total;
  for (int w = 0; w < wave; w++) base += wsum[w];
  if (tid == 0) pre[0] = 0;
  #pragma unroll
  for (int q = 0; q < 4; q++) if (tid * 4 + q < ns) pre[tid * 4 + q + 1] = base + run[q];
  for (int k = tid; k < n_rn; k += 1024) {
    const TreeNode nd = rn[k];
    if (!tree_node_ok (nd, ns)) bad |= 2;
    else atomicMax (&far[nd.first], nd.first + nd.size);
  }
  __syncthreads ();
  for (int k = wave; k < n_rn; k += 16) {               // a wavefront per node
    const TreeNode nd = rn[k];
    const bool ok = tree_node_ok (nd, ns);
    u64 kk = 0;
    if (ok) {
      const int end = nd.first + nd.size;
      int m = 0;
      for (int p = nd.first + 1 + lane; p < end; p += 64) m = max (m, far[p]);
      for (int o = 32; o; o >>= 1) m = max (m, __shfl_xor (m, o));
      if (m > end) bad |= 4;                            // a node that starts inside this one ends behind it
      kk = (u64) nd.size << CONS_KEY_BITS | ((pre[end] - pre[nd.first]) & key_mask);
    }
    if (lane == 0) { key[off + k] = kk; val[off + k] = (u32) (off + k); }
  }
  if (bad) { atomicOr (&rbad[r], bad); atomicOr (flags, bad); }
}

__global__ __launch_bounds__ (256)
void cons_heads_kernel (const u64 *__restrict__ key, long n, u32 *__restrict__ head, int *__restrict__ cls, int *__restrict__ cnt)
{
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    head[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
    cls[i] = -1; cnt[i] = 0;
  }
}

// (the run of sorted record i: the heads before it and its own, less one)
__device__ __forceinline__ u32 cons_run (const u32 *__restrict__ head, const u32 *__restrict__ hex, long i) { return hex[i] + head[i] - 1u; }

__global__ __launch_bounds__ (256)
void cons_lead_kernel (long n, const u32 *__restrict__ head, const u32 *__restrict__ hex, const int *__restrict__ cls, u32 *__restrict__ lead, const int *__restrict__ flags)
{
  if (*(volatile const int *) flags != 0) return;
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x)
    if (cls[i] < 0) atomicMin (&lead[cons_run (head, hex, i)], (u32) i);
}

__global__ __launch_bounds__ (256)
void cons_compare_kernel (ConsIn A, long n, const u32 *__restrict__ val, const u32 *__restrict__ head, const u32 *__restrict__ hex, const u32 *__restrict__ lead,
                          int *__restrict__ cls, int *__restrict__ flags)
{
  if (*(volatile const int *) flags != 0) return;
  const int lane = threadIdx.x & 63;
  for (long i = (blockIdx.x * (long) blockDim.x + threadIdx.x) >> 6; i < n; i += ((long) gridDim.x * blockDim.x) >> 6) {   // a wavefront per record
    if (cls[i] >= 0) continue;
    const long L = lead[cons_run (head, hex, i)];
    if (L == i) { if (lane == 0) cls[i] = (int) i; continue; }
    if (L < 0 || L >= n) continue;                      // (not taken: an unsettled record put an index of its run there)
    const int g = (int) val[i], gl = (int) val[L], r = A.rep_of (g), rl = A.rep_of (gl);
    const TreeNode nd = A.node_of (g, r), ld = A.node_of (gl, rl);
    bool equal = nd.size == ld.size;                    // (the key holds the size: taken)
    if (equal) {
      const int *const mem = A.members_of (rl, ld.first);
      const unsigned short *const pos = A.pos + (long) r * A.ns;
      int lo = CLD_MAX, hi = -1;
      for (int t = lane; t < ld.size; t += 64) { const int v = pos[mem[t]]; lo = min (lo, v); hi = max (hi, v); }
      for (int o = 32; o; o >>= 1) { lo = min (lo, __shfl_xor (lo, o)); hi = max (hi, __shfl_xor (hi, o)); }
      equal = hi - lo + 1 == nd.size && lo == nd.first; // the leader's members lie side by side in this replicate's order, and there this node lies
    }
    if (lane == 0) { if (equal) cls[i] = (int) L; else atomicOr (flags + 1, 1); }
  }
}

__global__ __launch_bounds__ (256)
void cons_count_kernel (ConsIn A, long n, const u32 *__restrict__ val, const u32 *__restrict__ head, const u32 *__restrict__ hex, const int *__restrict__ cls,
                        int *__restrict__ cnt, int *__restrict__ flags)
{
  if (*(volatile const int *) flags != 0) return;
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    const int L = cls[i];
    if (L < 0 || L >= n) continue;                      // (not taken: the rounds settle every record)
    const int r = A.rep_of ((int) val[i]);
    const u32 run = cons_run (head, hex, i);
    bool again = false;                                 // an earlier record of this replicate in this class: the replicate is counted there
    for (long j = i - 1; j >= 0 && !again && cons_run (head, hex, j) == run && A.rep_of ((int) val[j]) == r; j--) again = cls[j] == L;
    if (!again) atomicAdd (&cnt[L], 1);
    if (L == i) atomicAdd (flags + 3, 1);
  }
}

__global__ __launch_bounds__ (256)
void cons_kept_kernel (ConsIn A, long n, const u32 *__restrict__ val, const int *__restrict__ cls, const int *__restrict__ cnt, int min_count,
                       int *__restrict__ rep_count, int *__restrict__ kept, int *__restrict__ flags)
{
  if (*(volatile const int *) flags != 0) return;
  for (long i = blockIdx.x * (long) blockDim.x + threadIdx.x; i < n; i += (long) gridDim.x * blockDim.x) {
    const int L = cls[i];
    if (L < 0 || L >= n) continue;
    const int count = cnt[L];
    if (rep_count) {
      const int g = (int) val[i], r = A.rep_of (g);
      rep_count[(long) r * (A.ns - 1) + (g - A.rep_off[r])] = count;
    }
    if (L == i && count >= min_count) {
      const int slot = atomicAdd (flags + 2, 1);        // (any order: cons_order_kernel ranks them by a total order)
      if (slot < A.ns - 1) kept[slot] = (int) i;
    }
  }
}

__global__ __launch_bounds__ (256)
void cons_info_kernel (ConsIn A, const u32 *__restrict__ val, const int *__restrict__ cnt, const int *__restrict__ kept, ConsKept *__restrict__ info, const int *__restrict__ flags)
{
  if (*(volatile const int *) flags != 0) return;
  const int lane = threadIdx.x & 63, slot = (blockIdx.x * 256 + threadIdx.x) >> 6, nk = min (((volatile const int *) flags)[2], A.ns - 1);
  if (slot >= nk) return;
  const int i = kept[slot], g = (int) val[i], r = A.rep_of (g);
  const TreeNode nd = A.node_of (g, r);
  const int *const mem = A.members_of (r, nd.first);
  int m = CLD_MAX;
  for (int t = lane; t < nd.size; t += 64) m = min (m, mem[t]);
  for (int o = 32; o; o >>= 1) m = min (m, __shfl_xor (m, o));
  if (lane == 0) info[slot] = ConsKept {nd.size, m, cnt[i], r, nd.first, 0};
}

__global__ __launch_bounds__ (1024)
void cons_order_kernel (const ConsKept *__restrict__ info, ConsKept *__restrict__ sorted, int *__restrict__ leafpar, int ns, const int *__restrict__ flags)
{
  __shared__ u32 keys[CLD_MAX];
  if (*(volatile const int *) flags != 0) return;
  const int tid = threadIdx.x, nk = min (((volatile const int *) flags)[2], ns - 1);
  for (int s = tid; s < ns; s += 1024) leafpar[s] = CLD_MAX;
  for (int x = tid; x < nk; x += 1024) keys[x] = (u32) info[x].size << 12 | (u32) info[x].minm;
  __syncthreads ();
  for (int x = tid; x < nk; x += 1024) {
    const u32 mine = keys[x];
    int rank = 0;
    for (int j = 0; j < nk; j++) rank += (keys[j] < mine || (keys[j] == mine && j < x)) ? 1 : 0;
    sorted[rank] = info[x];
  }
}

__global__ __launch_bounds__ (256)
void cons_parent_kernel (ConsIn A, const ConsKept *__restrict__ sorted, int *__restrict__ kpar, int *__restrict__ leafpar, const int *__restrict__ flags)
{
  if (*(volatile const int *) flags != 0) return;
  const int lane = threadIdx.x & 63, j = (blockIdx.x * 256 + threadIdx.x) >> 6, nk = min (((volatile const int *) flags)[2], A.ns - 1);
  if (j >= nk) return;
  const ConsKept me = sorted[j];
  const int *const mem = A.members_of (me.rep, me.first);
  for (int t = lane; t < me.size; t += 64) atomicMin (&leafpar[mem[t]], j);   // the smallest kept class that holds the sample
  int par = -1;
  for (int b = j + 1; b < nk && par < 0; b += 64) {     // classes of the same size are disjoint from this one: the first larger one that holds its smallest member
    bool hit = false;
    if (b + lane < nk) {
      const ConsKept c = sorted[b + lane];
      if (c.size > me.size) { const int p = A.pos[(long) c.rep * A.ns + me.minm]; hit = p >= c.first && p < c.first + c.size; }
    }
    const u64 hits = __ballot (hit);
    if (hits) par = b + __ffsll ((long long) hits) - 1;
  }
  if (lane == 0) kpar[j] = par;
}

__global__ __launch_bounds__ (1024)
void cons_layout_kernel (const ConsKept *__restrict__ sorted, const int *__restrict__ kpar, const int *__restrict__ leafpar, int ns, ConsNode *__restrict__ nodes,
                         int *__restrict__ order, int *__restrict__ flags)
{
  // all of them by node or by sample; CONS_NONE: no parent
  __shared__ unsigned short par[CLD_MAX], siz[CLD_MAX], cur[CLD_MAX], fst[CLD_MAX], top[CLD_MAX], lpar[CLD_MAX], loff[CLD_MAX];
  if (*(volatile const int *) flags != 0) return;
  const int tid = threadIdx.x, n_kept = ((volatile const int *) flags)[2];
  if (n_kept > ns - 1) { if (tid == 0) flags[4] = 1; return; }
  const int nk = n_kept;
  for (int x = tid; x < nk; x += 1024) { par[x] = kpar[x] < 0 ? CONS_NONE : (unsigned short) kpar[x]; siz[x] = (unsigned short) sorted[x].size; cur[x] = 0; fst[x] = 0; }
  for (int t = tid; t < ns; t += 1024) { top[t] = CONS_NONE; lpar[t] = leafpar[t] >= nk ? CONS_NONE : (unsigned short) leafpar[t]; loff[t] = 0; }
  __syncthreads ();
  // The nodes whose smallest member is t are nested; the largest of them, top[t], is the one whose parent starts elsewhere.
  // Every other one is its parent's first child, and so is the sample t in the smallest of them: cur[] of a node starts
  // behind its first child.
  for (int x = tid; x < nk; x += 1024) {
    const int P = kpar[x];
    if (P < 0 || sorted[P].minm != sorted[x].minm) top[sorted[x].minm] = (unsigned short) x;
    else cur[P] = siz[x];
  }
  __syncthreads ();
  for (int t = tid; t < ns; t += 1024) if (top[t] != CONS_NONE && lpar[t] != CONS_NONE) cur[lpar[t]] = 1;   // (lpar[t] is a node: top[t] holds t)
  __syncthreads ();
  if (tid == 0) {
    int roots = 0;                                      // the samples in ascending order: what starts at t takes the next place in its parent
    for (int t = 0; t < ns; t++) {
      const int x = top[t];
      if (x != CONS_NONE) {
        const int P = par[x];
        if (P == CONS_NONE) { fst[x] = (unsigned short) roots; roots += siz[x]; } else { fst[x] = cur[P]; cur[P] = (unsigned short) (cur[P] + siz[x]); }
      } else {
        const int P = lpar[t];
        if (P == CONS_NONE) { loff[t] = (unsigned short) roots; roots += 1; } else { loff[t] = cur[P]; cur[P] = (unsigned short) (cur[P] + 1); }
      }
    }
    for (int x = nk - 1; x >= 0; x--)                   // a parent comes behind its children: from the back, its first is final
      if (par[x] != CONS_NONE) fst[x] = (unsigned short) (fst[x] + fst[par[x]]);
  }
  __syncthreads ();
  for (int x = tid; x < nk; x += 1024) nodes[x] = ConsNode {kpar[x], sorted[x].count, (int) fst[x], (int) siz[x]};
  for (int t = tid; t < ns; t += 1024) {
    const int at = (lpar[t] == CONS_NONE ? 0 : (int) fst[lpar[t]]) + (int) loff[t];
    if (at < ns) order[at] = t;
  }
}

extern "C" long tjamd_consensus_tree (tjamd_counter *c, const tjamd_tree_node *d_rep_nodes, const int *d_rep_order, const int *h_rep_n_nodes, int n_samples, int n_replicates,
                                      int min_count, tjamd_consensus_node *d_nodes, int *d_order, int *d_rep_count, long *h_n_classes)
{
  static const char *fn = "tjamd_consensus_tree";
  if (!c) return -set_err (TJAMD_ERR_ARG, "%s: null counter", fn);
  if (!d_rep_order) return -set_err (TJAMD_ERR_ARG, "%s: null d_rep_order", fn);
  if (!h_rep_n_nodes) return -set_err (TJAMD_ERR_ARG, "%s: null h_rep_n_nodes", fn);
  if (!d_order) return -set_err (TJAMD_ERR_ARG, "%s: null d_order", fn);
  if (n_samples < 1 || n_samples > CLD_MAX) return -set_err (TJAMD_ERR_ARG, "%s: n_samples %d outside 1..4096", fn, n_samples);
  if (const int bad = replicates_arg (fn, n_replicates)) return -bad;
  if (!d_nodes && n_samples > 1) return -set_err (TJAMD_ERR_ARG, "%s: null d_nodes", fn);
  long n = 0;                                           // the clades of the call
  if (const int bad = rep_nodes_args (fn, h_rep_n_nodes, n_replicates, n_samples, d_rep_nodes, &n)) return -bad;
  if (min_count > n_replicates || 2l * min_count <= n_replicates)
    return -set_err (TJAMD_ERR_ARG, "%s: min_count %d outside %d..%d (more than half of the %d replicates)", fn, min_count, n_replicates / 2 + 1, n_replicates, n_replicates);
  Stage st (c, T_CONSENSUS_TREE);                       // (a refused call leaves no timing behind)
  if (const int bad = st.enter (fn, "the clades are classed")) return -bad;
  const int ns = n_samples, R = n_replicates;
  int rc;
  if (ns == 1) {                                        // one sample: no clade, no kernel
    if (hipMemsetAsync (d_order, 0, sizeof (int), c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: memset failed", fn);
    rc = read_back (c, fn, nullptr, nullptr, 0);
    if (rc) return -rc;
    if (h_n_classes) *h_n_classes = 0;
    return 0;
  }
  std::vector<int> h_rep ((size_t) 2 * R + 1);          // the counts, and where each replicate's records start
  for (int r = 0, at = 0; r < R; r++) { h_rep[r] = h_rep_n_nodes[r]; h_rep[R + r] = at; at += h_rep_n_nodes[r]; }
  h_rep[2 * R] = (int) n;
  const size_t n1 = (size_t) std::max (n, 1l);
  ScratchCut cut;
  u64 *key[2]; u32 *val[2], *head, *hex, *lead; int *cls, *cnt, *reps, *rbad, *kept, *kpar, *flags; unsigned short *pos; ConsKept *info;
  cut.take (key[0], n1); cut.take (key[1], n1); cut.take (val[0], n1); cut.take (val[1], n1); cut.take (head, n1); cut.take (hex, n1); cut.take (lead, n1);
  cut.take (cls, n1); cut.take (cnt, n1); cut.take (pos, (size_t) R * ns); cut.take (reps, (size_t) 2 * R + 1); cut.take (rbad, (size_t) R);
  cut.take (kept, (size_t) ns); cut.take (kpar, (size_t) 2 * ns); cut.take (info, (size_t) 2 * ns);
  rc = commit_with_flags (cut, c, fn, flags);
  if (!rc) rc = reserve_sort (c, (long) n1, (long) n1);
  if (rc) return -rc;
  ConsKept *const sorted = info + ns; int *const leafpar = kpar + ns;
  if (hipMemsetAsync (rbad, 0, (size_t) R * sizeof (int), c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: memset failed", fn);
  if (hipMemcpyAsync (reps, h_rep.data (), h_rep.size () * sizeof (int), hipMemcpyHostToDevice, c->stream) != hipSuccess) return -set_err (TJAMD_ERR_HIP, "%s: copy failed", fn);
  ConsIn A;
  A.rep_nodes = (const TreeNode *) d_rep_nodes; A.rep_order = d_rep_order; A.rep_n = reps; A.rep_off = reps + R; A.pos = pos; A.ns = ns; A.R = R;
  const u64 key_mask = (1ull << c->consensus_key_bits) - 1ull;
  const unsigned wave_grid = (unsigned) std::max<long> (1, std::min<long> ((n + 3) / 4, 16l * c->n_cu)), kept_grid = (unsigned) ((ns - 1 + 3) / 4);
  u32 h_flags[5] = {0, 0, 0, 0, 0};
  st.begin ();
  hipLaunchKernelGGL (cons_records_kernel, dim3 ((unsigned) R), dim3 (1024), 0, c->stream, A, key_mask, pos, key[0], val[0], rbad, flags);
  if (n > 0) {
    rc = kv_sort (c, key, val, n, 64);
    if (rc) return -rc;
    hipLaunchKernelGGL (cons_heads_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, (const u64 *) key[0], n, head, cls, cnt);
    rc = exclusive_scan (c, head, hex, n, nullptr);
    if (rc) return -rc;
    for (long round = 0; ; round++) {                   // a round settles the leader of every run that has an unsettled record: n rounds at the very most
      if (round > n) return -set_err (TJAMD_ERR_STATE, "%s: the rounds did not end", fn);
      if (hipMemsetAsync (flags + 1, 0, sizeof (int), c->stream) != hipSuccess || hipMemsetAsync (lead, 0xFF, (size_t) n * sizeof (u32), c->stream) != hipSuccess)
        return -set_err (TJAMD_ERR_HIP, "%s: memset failed", fn);
      hipLaunchKernelGGL (cons_lead_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, n, (const u32 *) head, (const u32 *) hex, (const int *) cls, lead, (const int *) flags);
      hipLaunchKernelGGL (cons_compare_kernel, dim3 (wave_grid), dim3 (256), 0, c->stream, A, n, (const u32 *) val[0], (const u32 *) head, (const u32 *) hex, (const u32 *) lead, cls, flags);
      st.end ();
      rc = read_back (c, fn, flags, h_flags, 2);
      if (rc) return -rc;
      if (h_flags[0] || !h_flags[1]) break;
    }
    hipLaunchKernelGGL (cons_count_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, A, n, (const u32 *) val[0], (const u32 *) head, (const u32 *) hex, (const int *) cls, cnt, flags);
    hipLaunchKernelGGL (cons_kept_kernel, dim3 (grid_for (n)), dim3 (256), 0, c->stream, A, n, (const u32 *) val[0], (const int *) cls, (const int *) cnt, min_count, d_rep_count, kept, flags);
    hipLaunchKernelGGL (cons_info_kernel, dim3 (kept_grid), dim3 (256), 0, c->stream, A, (const u32 *) val[0], (const int *) cnt, (const int *) kept, info, (const int *) flags);
  }
  hipLaunchKernelGGL (cons_order_kernel, dim3 (1), dim3 (1024), 0, c->stream, (const ConsKept *) info, sorted, leafpar, ns, (const int *) flags);
  if (n > 0) hipLaunchKernelGGL (cons_parent_kernel, dim3 (kept_grid), dim3 (256), 0, c->stream, A, (const ConsKept *) sorted, kpar, leafpar, (const int *) flags);
  hipLaunchKernelGGL (cons_layout_kernel, dim3 (1), dim3 (1024), 0, c->stream, (const ConsKept *) sorted, (const int *) kpar, (const int *) leafpar, ns, (ConsNode *) d_nodes, d_order, flags);
  st.end ();
  rc = read_back (c, fn, flags, h_flags, 5);
  if (rc) return -rc;
  if (h_flags[0]) {                                     // the smallest refused replicate, its first broken rule in the header's order
    std::vector<int> h_bad ((size_t) R, 0);
    rc = read_back (c, fn, rbad, h_bad.data (), (size_t) R);
    if (rc) return -rc;
    for (int r = 0; r < R; r++) {
      const int bad = h_bad[r];
      if (bad & 1) return -set_err (TJAMD_ERR_ARG, "%s: the order of replicate %d is not a permutation of 0 .. n_samples - 1", fn, r);
      if (bad & 2) return -set_err (TJAMD_ERR_ARG, "%s: a node of replicate %d has size < 2, first < 0 or first + size above n_samples %d", fn, r, ns);
      if (bad & 4) return -set_err (TJAMD_ERR_ARG, "%s: two nodes of replicate %d cross (they overlap and neither contains the other)", fn, r);
    }
    return -set_err (TJAMD_ERR_STATE, "%s: an error word without a replicate", fn);
  }
  if (h_flags[4]) return -set_err (TJAMD_ERR_STATE, "%s: %u kept classes on %d samples", fn, h_flags[2], ns);
  st.done ();
  if (h_n_classes) *h_n_classes = (long) h_flags[3];
  return (long) h_flags[2];
}
TJ_LAST_MS (tjamd_last_consensus_tree_ms, T_CONSENSUS_TREE)

// ---------------------------------------------------------------------------------------------------------------
// Plain FASTQ text parsed on the device (tjamd_fastq_*; the rule: include/tatajuba_amd.h).
//
// A push sees a logical text: the carry region of `cap` bytes (a multiple of FQ_TILE; the carried tail lies at its end, from
// FqState::start on) and behind it the pushed bytes where they lie, so a 16-byte chunk and a tile are in one of the two.  The
// host knows bounds only (the carry is at most what the push before could see, or what a look-back that has arrived says;
// the stream at most half the text), sizes every grid and buffer from them, and waits for nothing before tjamd_fastq_end;
// what a kernel needs of the device's own numbers it takes from FqState, which the kernel before it wrote.  Per push: fq_count_kernel (line ends per tile, the first '\r'),
// a scan of the tile counts, fq_lines_kernel (the line ends as 32-bit offsets), fq_check_kernel (one lane per record of four
// lines: the rule, len (L1) + 1), a scan of those lengths, fq_finish_kernel (one lane: the consumed prefix, the stop, the
// session's sums), fq_copy_kernel (the stream, by output position: 16 bytes a lane whatever the read lengths are) and
// fq_carry_kernel (the tail, into the other of two carry buffers).  No workgroup waits for another: kernel boundaries order it all.

#define FQ_TILE   4096                  // text bytes of one workgroup: 256 lanes x 16 bytes (a wavefront spans 1024)
#define FQ_BLOCK  256
#define FQ_MAX_PUSH (1ull << 30)
#define FQ_STAGE_BYTES (8u << 20)       // tjamd_fastq_push_host from pageable memory: two pinned buffers of this size
#define FQ_SCAN_BATCH (16u << 20)       // a session that scans hands its stream on when this many bytes may have gathered (every push of 32 MiB of text and more)
#define FQ_TIMED_PUSHES 1024            // pushes of a session with an event pair of their own; a longer session has no time
#define FQ_LOOKS  8
#define FQ_NONE   0xFFFFFFFFu

struct FqState
{ // (device; tjamd_fastq_end copies it to the host)
  u32 start;                            // logical offset of the first byte not yet consumed (cap: no carry)
  u32 stop;
  u32 n_lines;                          // line ends of this push from start on
  u32 first_bad, first_cr, big0;        // this push: the first irregular record, the first '\r', record 0 began in the carry and outgrew it
  u32 n_good, push_stream;              // records this push consumed, their stream bytes
  u32 new_pos, tail_len;                // where the unconsumed tail starts, and its length
  u64 consumed, reads, stream_total;    // of the session
  u64 stream_fill, stream_base;         // bytes in the stream buffer; where this push's bytes begin in it
};

struct FqSrc { const uint8_t *carry, *text; u32 cap, lo, end; int final; };   // tiles start at lo; end = cap + the push's bytes

__device__ __forceinline__ u32 fq_byte (const FqSrc &S, u32 p) { return p < S.cap ? S.carry[p] : S.text[p - S.cap]; }

// bit i: byte p0 + i of the logical text, in [start, end), is a line end -- a '\n', or the end of a final text whose last
// byte is none (the bit of position `end`); cr: the same for '\r'
__device__ __forceinline__ u32 fq_chunk_masks (const FqSrc &S, u32 p0, u32 start, u32 &cr)
{
  u32 nl = 0;
  cr = 0;
  if (p0 < S.end && p0 + 16 > start) {
    const uint4 v = *(const uint4 *) (p0 < S.cap ? S.carry + p0 : S.text + (p0 - S.cap));
    const u32 w[4] = {v.x, v.y, v.z, v.w};
    #pragma unroll
    for (int j = 0; j < 4; j++) {
      #pragma unroll
      for (int b = 0; b < 4; b++) {
        const u32 ch = (w[j] >> (8 * b)) & 0xFFu;
        nl |= (u32) (ch == (u32) '\n') << (4 * j + b);
        cr |= (u32) (ch == (u32) '\r') << (4 * j + b);
      }
    }
    u32 keep = 0xFFFFu;
    if (start > p0) keep &= 0xFFFFu << (start - p0);
    if (S.end - p0 < 16) keep &= (1u << (S.end - p0)) - 1u;
    nl &= keep; cr &= keep;
  }
  if (S.final && S.end > start && (S.end & ~15u) == p0 && fq_byte (S, S.end - 1) != (u32) '\n') nl |= 1u << (S.end - p0);
  return nl;
}

__global__ void fq_begin_kernel (FqState *st, u32 cap)
{
  FqState z = {};
  z.start = cap; z.first_bad = z.first_cr = FQ_NONE;
  *st = z;
}

__global__ __launch_bounds__ (FQ_BLOCK)
void fq_count_kernel (FqSrc S, FqState *st, u32 *__restrict__ tile_count)
{
  __shared__ u32 s_tmp[4];
  if (st->stop) return;
  const u32 p0 = S.lo + blockIdx.x * FQ_TILE + threadIdx.x * 16u;
  u32 cr;
  const u32 nl = fq_chunk_masks (S, p0, st->start, cr);
  u32 total;
  block_exclusive_scan_256 (__popc (nl), s_tmp, total);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
  if (cr) { const u32 at = p0 + (u32) __ffs (cr) - 1u; if (at < st->first_cr) atomicMin (&st->first_cr, at); }
}

__global__ __launch_bounds__ (FQ_BLOCK)
void fq_lines_kernel (FqSrc S, const FqState *st, const u32 *__restrict__ tile_base, u32 *__restrict__ lineend, u32 lcap)
{
  __shared__ u32 s_tmp[4];
  if (st->stop) return;
  const u32 p0 = S.lo + blockIdx.x * FQ_TILE + threadIdx.x * 16u;
  u32 cr, nl = fq_chunk_masks (S, p0, st->start, cr);
  u32 total;
  u32 rank = tile_base[blockIdx.x] + block_exclusive_scan_256 (__popc (nl), s_tmp, total);
  while (nl) {
    if (rank < lcap) lineend[rank] = p0 + (u32) __ffs (nl) - 1u;
    rank++; nl &= nl - 1u;
  }
}

// one lane per record r of the first lcap line ends (lcap / 4 = rb records at most; more lines than lcap: a record among
// these is irregular, since rb regular records are longer than the text): the rule, and len[r] = len (L1) + 1, 0 from the
// last whole record on, up to and including r = rb
__global__ void fq_check_kernel (FqSrc S, FqState *st, const u32 *__restrict__ lineend, u32 lcap, u32 rb, u32 carry_max, u32 *__restrict__ len)
{
  const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > rb || st->stop) return;
  const u32 n_rec = min (st->n_lines, lcap) >> 2;
  u32 l = 0;
  if (r < n_rec) {
    const u32 s0 = r ? lineend[4 * r - 1] + 1u : st->start;
    const u32 e0 = lineend[4 * r], e1 = lineend[4 * r + 1], e2 = lineend[4 * r + 2], e3 = lineend[4 * r + 3];
    const u32 l1 = e1 - e0 - 1u, l3 = e3 - e2 - 1u, cr = st->first_cr;
    bool ok = fq_byte (S, s0) == (u32) '@' && l1 >= 1u && l3 == l1 && !(cr >= s0 && cr <= e3);   // (an empty line's first byte is its '\n', never the text's end)
    if (ok) { const u32 ch = fq_byte (S, e0 + 1u); ok = ch != (u32) '>' && ch != (u32) '+' && ch != (u32) '@' && fq_byte (S, e1 + 1u) == (u32) '+'; }
    if (!ok && r < st->first_bad) atomicMin (&st->first_bad, r);
    if (r == 0 && s0 < S.cap && min (e3 + 1u, S.end) - s0 > carry_max) st->big0 = 1u;   // cut by a push boundary and longer than the carry
    l = l1 + 1u;
  }
  len[r] = l;
}

__global__ void fq_finish_kernel (FqSrc S, FqState *st, const u32 *__restrict__ lineend, const u32 *__restrict__ off, u32 lcap, u32 carry_max, int flush)
{ // flush: the stream buffer is handed to the scan behind this push, the next push's bytes begin at its start
  if (threadIdx.x || blockIdx.x) return;
  st->stream_base = st->stream_fill;
  if (st->stop) { st->n_good = 0; st->push_stream = 0; if (flush) st->stream_fill = 0; return; }
  const u32 n_rec = min (st->n_lines, lcap) >> 2, bad = st->big0 ? 0u : st->first_bad;
  const u32 n_good = min (bad, n_rec);
  const u32 new_pos = n_good ? min (lineend[4 * n_good - 1] + 1u, S.end) : st->start;
  const u32 tail = S.end - new_pos, grown = off[n_good];
  u32 stop = 0;
  if (st->big0) stop = 2;
  else if (bad < n_rec) stop = 1;
  else if (!S.final && tail > carry_max) stop = 2;
  st->consumed += new_pos - st->start; st->reads += n_good; st->stream_total += grown;
  st->stream_fill = flush ? 0ull : st->stream_fill + grown;
  st->n_good = n_good; st->push_stream = grown; st->new_pos = new_pos; st->tail_len = tail; st->stop = stop;
  st->start = (stop || S.final) ? S.cap : S.cap - tail;
  st->first_bad = st->first_cr = FQ_NONE; st->big0 = 0;
}

// the largest r in [lo, hi] with off[r] <= o (off[lo] <= o)
__device__ __forceinline__ u32 fq_record_of (const u32 *__restrict__ off, u32 lo, u32 hi, u32 o)
{
  while (lo < hi) { const u32 mid = (lo + hi + 1u) >> 1; if (off[mid] <= o) lo = mid; else hi = mid - 1u; }
  return lo;
}

// The stream by output position: a lane makes the 16 bytes at one 16-byte line of the stream buffer, from whichever records
// they come, and stores them at once (byte by byte on the push's first and last line).  pad_to != 0 (scan sessions): every
// byte from the data's end to pad_to is a '\n', so that the scan can take the host's bound for the length.
__global__ __launch_bounds__ (256)
void fq_copy_kernel (FqSrc S, const FqState *st, const u32 *__restrict__ lineend, const u32 *__restrict__ len, const u32 *__restrict__ off,
                     uint8_t *__restrict__ stream, u64 pad_to)
{
  __shared__ u32 s_r[2];
  const u64 base = st->stream_base, data_hi = base + st->push_stream, w_hi = pad_to ? pad_to : data_hi;
  const u32 n_good = st->n_good;
  const u64 a_blk = (base & ~15ull) + (u64) blockIdx.x * 4096ull;
  if (a_blk >= w_hi) return;
  const bool has_data = n_good && a_blk < data_hi;
  if (has_data && threadIdx.x < 2) {
    const u64 a = threadIdx.x ? min (a_blk + 4096ull, data_hi) - 1ull : max (a_blk, base);
    s_r[threadIdx.x] = fq_record_of (off, 0u, n_good - 1u, (u32) (a - base));
  }
  __syncthreads ();
  const u64 a0 = a_blk + 16ull * threadIdx.x;
  if (a0 >= w_hi || a0 + 16ull <= base) return;
  u32 r = 0, j = 0, l = 0, p = 0;
  const u64 a_first = max (a0, base);
  if (has_data && a_first < data_hi) {
    const u32 o = (u32) (a_first - base);
    r = fq_record_of (off, s_r[0], s_r[1], o);
    j = o - off[r]; l = len[r]; p = lineend[4 * r] + 1u + j;
  }
  u32 w[4] = {0u, 0u, 0u, 0u};
  #pragma unroll
  for (int i = 0; i < 16; i++) {
    const u64 a = a0 + (u64) i;
    u32 ch = (u32) '\n';
    if (a >= base && a < data_hi) {
      if (j + 1u < l) ch = fq_byte (S, p);
      j++; p++;
      if (j == l) { r++; j = 0; if (r < n_good) { l = len[r]; p = lineend[4 * r] + 1u; } }
    }
    w[i >> 2] |= ch << (8 * (i & 3));
  }
  if (a0 >= base && a0 + 16ull <= w_hi) *(uint4 *) (stream + a0) = make_uint4 (w[0], w[1], w[2], w[3]);
  else {
    #pragma unroll
    for (int i = 0; i < 16; i++) { const u64 a = a0 + (u64) i; if (a >= base && a < w_hi) stream[a] = (uint8_t) (w[i >> 2] >> (8 * (i & 3))); }
  }
}

__global__ void fq_carry_kernel (FqSrc S, const FqState *st, uint8_t *__restrict__ next_carry)
{ // the tail [new_pos, new_pos + tail_len) to the end of the other carry buffer
  if (st->stop || S.final) return;
  const u32 tail = st->tail_len, from = st->new_pos, to = S.cap - tail;
  const u32 i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 16u;
  for (u32 i = i0; i < min (i0 + 16u, tail); i++) next_carry[to + i] = (uint8_t) fq_byte (S, from + i);
}

struct FastqSession
{
  bool open = false, final_seen = false, ended = false;
  int m = -1;                                           // -1: parse only
  u32 cap = 0;                                          // the carry region: the counter's carry limit rounded up to tiles
  // What the host knows.  The carry is at most carry_bound: what the push before could see, and less once a look-back has
  // arrived (below).  The stream in the buffer comes from text_since bytes at most -- the carry bound when the buffer was
  // last handed to the scan, plus every byte pushed since -- so it is at most half of them: a bound of the session, which
  // the number of pushes does not enter.
  size_t carry_bound = 0, text_since = 0, stream_bound = 0, pushed = 0;
  // look-backs: behind every push the state block is copied to one of FQ_LOOKS pinned slots, and a later push takes from the
  // slots whose copy has arrived (asked without waiting) the tail that push left: the carry is at most that plus what was
  // pushed since.  Without them the bound could only rise, to the carry's limit, and stay there whatever the pushes hold.
  FqState *look = nullptr; hipEvent_t look_ev[FQ_LOOKS] = {}; bool look_used[FQ_LOOKS] = {}; size_t look_pushed[FQ_LOOKS] = {};
  bool seen_stop = false;
  int cur = 0;                                          // which carry buffer the next push reads
  DevBuf carry[2], state, text, stream;
  void *pin[2] = {nullptr, nullptr}; hipEvent_t pin_ev[2] = {nullptr, nullptr}; bool pin_used[2] = {false, false}; int pin_next = 0;
  std::vector<hipEvent_t> ev;                           // pairs around the parse kernels of the pushes
  long n_push = 0;
  long consumed = -1, reads = 0, stream_bytes = 0; int stop = 0; bool kept = false; double ms = -1.0;
};

static void fastq_release (tjamd_counter *c)
{
  FastqSession *q = c->fq;
  if (!q) return;
  DevBuf *all[] = {&q->carry[0], &q->carry[1], &q->state, &q->text, &q->stream};
  for (DevBuf *b : all) release (*b);
  for (int i = 0; i < 2; i++) { if (q->pin[i]) (void) hipHostFree (q->pin[i]); if (q->pin_ev[i]) (void) hipEventDestroy (q->pin_ev[i]); }
  for (hipEvent_t e : q->ev) (void) hipEventDestroy (e);
  for (hipEvent_t e : q->look_ev) if (e) (void) hipEventDestroy (e);
  if (q->look) (void) hipHostFree (q->look);
  delete q;
  c->fq = nullptr;
}

extern "C" int tjamd_fastq_tile_bytes (void) { return FQ_TILE; }
// diagnostic (tests, tools): the sessions this process has ended -- how a run of the drop-in shows which way its file went
static long g_fastq_sessions = 0;
extern "C" long tjamd_debug_fastq_sessions (void) { return __atomic_load_n (&g_fastq_sessions, __ATOMIC_RELAXED); }

// The counter of this thread's last call that was refused before the counter was read (it may be no counter at all: the
// pointer is compared, never followed): tjamd_last_fastq_ms gives -1.0 for it until a call on it gets through.
static thread_local const tjamd_counter *g_fastq_refused = nullptr;

static int fastq_host_refusal (const char *fn, tjamd_counter *c, const void *text, size_t n_bytes, bool device_text, int min_tract_size)
{
  if (!c) return set_err (TJAMD_ERR_ARG, "%s: TJAMD_ERR_ARG: null counter", fn);
  if (!text && n_bytes) return set_err (TJAMD_ERR_ARG, "%s: TJAMD_ERR_ARG: null text with n_bytes %zu", fn, n_bytes);
  if (n_bytes > FQ_MAX_PUSH) return set_err (TJAMD_ERR_ARG, "%s: TJAMD_ERR_ARG: n_bytes %zu above 1 GiB (push the text in pieces)", fn, n_bytes);
  if (device_text && ((uintptr_t) text & 15u)) return set_err (TJAMD_ERR_ARG, "%s: TJAMD_ERR_ARG: d_text must be 16-byte aligned", fn);
  if (min_tract_size < -1) return set_err (TJAMD_ERR_ARG, "%s: TJAMD_ERR_ARG: min_tract_size %d below -1", fn, min_tract_size);
  if (tjamd_device_count () <= 0) return set_err (TJAMD_ERR_NO_DEVICE, "%s: TJAMD_ERR_NO_DEVICE: no HIP device visible (the text is parsed on the device; no CPU fallback)", fn);
  return TJAMD_OK;
}

// the refusals of a call that need no device, then the one without a device, then the counter's device
static int fastq_enter (const char *fn, tjamd_counter *c, const void *text, size_t n_bytes, bool device_text, int min_tract_size)
{
  const int rc = fastq_host_refusal (fn, c, text, n_bytes, device_text, min_tract_size);
  if (rc) { g_fastq_refused = c; return rc; }
  if (g_fastq_refused == c) g_fastq_refused = nullptr;
  if (c->fq) c->fq->ms = -1.0;                          // (a refused call leaves no timing behind: tjamd_fastq_end sets it again)
  return hipSetDevice (c->device) == hipSuccess ? TJAMD_OK : set_err (TJAMD_ERR_HIP, "hipSetDevice failed");
}

// the look-backs that have arrived: a smaller carry bound, and whether the session is known to have stopped
static void fastq_look_back (FastqSession *q, u32 carry_max)
{
  for (int i = 0; i < FQ_LOOKS; i++) {
    if (!q->look_used[i] || hipEventQuery (q->look_ev[i]) != hipSuccess) continue;
    const FqState &h = q->look[i];
    if (h.stop) q->seen_stop = true;
    const size_t tail = (h.stop ? 0 : (size_t) h.tail_len) + (q->pushed - q->look_pushed[i]);
    q->carry_bound = std::min (q->carry_bound, std::min ((size_t) carry_max, tail));
    q->look_used[i] = false;
  }
  (void) hipGetLastError ();                            // (a copy that has not arrived is an error to hipEventQuery, not to the call)
}

// (hopo_host.c, not exported: a session that is known to have stopped takes no more text in)
extern "C" int tj_fastq_seen_stop (tjamd_counter *c)
{
  if (!c || !c->fq || !c->fq->open || hipSetDevice (c->device) != hipSuccess) return 0;
  fastq_look_back (c->fq, (u32) c->fastq_carry_max);
  return c->fq->seen_stop ? 1 : 0;
}

// diagnostic (tests): what a counter's sessions hold on to -- 0: bytes of the stream buffer, 1: bytes of the scratch block
// the pushes cut up, 2: the bound of the raw records that sizes their storage
extern "C" long tjamd_debug_fastq_footprint (const tjamd_counter *c, int what)
{
  if (!c) return -1;
  return what == 0 ? (c->fq ? (long) c->fq->stream.cap : 0) : what == 1 ? (long) c->lc_work.cap : what == 2 ? (long) c->raw_bound : -1;
}

extern "C" int tjamd_fastq_begin (tjamd_counter *c, int min_tract_size)
{
  static const char *fn = "tjamd_fastq_begin";
  int rc = fastq_enter (fn, c, nullptr, 0, false, min_tract_size);
  if (rc) return rc;
  if (c->fq && c->fq->open) return set_err (TJAMD_ERR_ARG, "%s: TJAMD_ERR_ARG: a session is open on this counter (tjamd_fastq_end closes it)", fn);
  if (min_tract_size >= 0 && (rc = check_scan_args (c, min_tract_size))) return rc;
  if (!c->fq) c->fq = new FastqSession ();
  FastqSession *q = c->fq;
  q->cap = (u32) (((size_t) c->fastq_carry_max + FQ_TILE - 1) / FQ_TILE * FQ_TILE);
  for (int i = 0; i < 2 && !rc; i++) rc = ensure (q->carry[i], q->cap, c->stream);
  if (!rc) rc = ensure (q->state, sizeof (FqState), c->stream);
  if (rc) return rc;
  if (!q->look) {
    HIPCHK (hipHostMalloc ((void **) &q->look, FQ_LOOKS * sizeof (FqState), hipHostMallocDefault));
    for (hipEvent_t &e : q->look_ev) HIPCHK (hipEventCreateWithFlags (&e, hipEventDisableTiming));
  }
  hipLaunchKernelGGL (fq_begin_kernel, dim3 (1), dim3 (1), 0, c->stream, (FqState *) q->state.p, q->cap);
  HIPCHK (hipGetLastError ());
  q->open = true; q->final_seen = false; q->ended = false; q->m = min_tract_size;
  q->carry_bound = 0; q->text_since = 0; q->stream_bound = 0; q->pushed = 0; q->cur = 0; q->n_push = 0; q->seen_stop = false;
  for (bool &u : q->look_used) u = false;               // (the last session's end waited for its copies)
  return TJAMD_OK;
}

// One push of an open session.  A session that scans gathers its stream in the buffer as one that parses only does, and
// hands it to the scan when FQ_SCAN_BATCH bytes may have gathered, on the final push and (`hand_on`) at the session's end:
// every scan launch adds a worst case of its own to the bounds that size the counter's record storage, which thousands of
// small pushes would run out of memory on.
static int fastq_push (tjamd_counter *c, const void *d_text, size_t n_bytes, int final, bool hand_on)
{
  FastqSession *q = c->fq;
  int rc;
  const u32 cap = q->cap, carry_max = (u32) c->fastq_carry_max;
  fastq_look_back (q, carry_max);
  const size_t avail = q->carry_bound + n_bytes;        // text this push can see, at most
  if (avail == 0 && !hand_on) return TJAMD_OK;
  FqSrc S;
  S.carry = (const uint8_t *) q->carry[q->cur].p; S.text = (const uint8_t *) d_text; S.cap = cap;
  S.lo = cap - (u32) ((q->carry_bound + FQ_TILE - 1) / FQ_TILE * FQ_TILE); S.end = cap + (u32) n_bytes; S.final = final ? 1 : 0;
  const long n_tiles = (long) ((S.end - S.lo) / FQ_TILE) + 1;
  const u32 rb = (u32) (avail / 8 + 1), lcap = 4u * rb;  // a regular record is eight bytes or more
  const size_t grown = avail / 2 + 16;                  // ... and gives at most half of them to the stream: this push's share
  const bool keep = q->m < 0;
  const size_t had = q->stream_bound, bound = (q->text_since + n_bytes) / 2 + 16, need = (bound + 15) & ~(size_t) 15;   // the buffer's, behind this push
  const bool flush = !keep && (hand_on || final || bound >= FQ_SCAN_BATCH);
  rc = ensure (q->stream, need + 256, c->stream, std::min (had, q->stream.cap));
  if (rc) return rc;
  ScratchCut cut;
  u32 *tile_count, *tile_base, *lineend, *len, *off, *tmp;
  const size_t tmp_words = scan_tmp_words (std::max<long> (n_tiles, (long) rb + 1));
  cut.take (tile_count, (size_t) n_tiles); cut.take (tile_base, (size_t) n_tiles); cut.take (lineend, (size_t) lcap);
  cut.take (len, (size_t) rb + 1); cut.take (off, (size_t) rb + 1); cut.take (tmp, tmp_words);
  rc = cut.commit (c);
  if (rc) return rc;
  FqState *st = (FqState *) q->state.p;
  const bool timed = q->n_push < FQ_TIMED_PUSHES;
  if (timed) {
    while (q->ev.size () < (size_t) (2 * q->n_push + 2)) { hipEvent_t e; HIPCHK (hipEventCreate (&e)); q->ev.push_back (e); }
    HIPCHK (hipEventRecord (q->ev[2 * q->n_push], c->stream));
  }
  hipLaunchKernelGGL (fq_count_kernel, dim3 ((unsigned) n_tiles), dim3 (FQ_BLOCK), 0, c->stream, S, st, tile_count);
  rc = exclusive_scan (c, tile_count, tile_base, n_tiles, &st->n_lines, tmp, tmp_words);
  if (rc) return rc;
  hipLaunchKernelGGL (fq_lines_kernel, dim3 ((unsigned) n_tiles), dim3 (FQ_BLOCK), 0, c->stream, S, (const FqState *) st, (const u32 *) tile_base, lineend, lcap);
  hipLaunchKernelGGL (fq_check_kernel, dim3 (rb / 256 + 1), dim3 (256), 0, c->stream, S, st, (const u32 *) lineend, lcap, rb, carry_max, len);
  rc = exclusive_scan (c, len, off, (long) rb + 1, nullptr, tmp, tmp_words);
  if (rc) return rc;
  hipLaunchKernelGGL (fq_finish_kernel, dim3 (1), dim3 (64), 0, c->stream, S, st, (const u32 *) lineend, (const u32 *) off, lcap, carry_max, flush ? 1 : 0);
  // (the copy's first line may begin up to 15 bytes in front of the push's first byte: one block more than the bytes need;
  // a push that pads the buffer for the scan does not know where its bytes begin, and takes blocks for all of it)
  hipLaunchKernelGGL (fq_copy_kernel, dim3 ((unsigned) (((flush ? need : grown) + 15) / 4096 + 2)), dim3 (256), 0, c->stream, S, (const FqState *) st, (const u32 *) lineend, (const u32 *) len,
                      (const u32 *) off, (uint8_t *) q->stream.p, flush ? (u64) need : 0ull);
  if (!final) {
    const size_t carry_next = std::min ((size_t) carry_max, avail);
    hipLaunchKernelGGL (fq_carry_kernel, dim3 ((unsigned) std::max<size_t> (1, (carry_next + 4095) / 4096)), dim3 (256), 0, c->stream, S, (const FqState *) st, (uint8_t *) q->carry[q->cur ^ 1].p);   // (nothing in sight: one workgroup that finds no tail)
    q->carry_bound = carry_next; q->cur ^= 1;
  }
  else q->carry_bound = 0;
  HIPCHK (hipGetLastError ());
  if (timed) HIPCHK (hipEventRecord (q->ev[2 * q->n_push + 1], c->stream));
  q->pushed += n_bytes;
  const int slot = (int) (q->n_push % FQ_LOOKS);         // (a slot whose copy is still on its way is left alone: this push leaves no look-back)
  if (!q->look_used[slot]) {
    HIPCHK (hipMemcpyAsync (&q->look[slot], st, sizeof (FqState), hipMemcpyDeviceToHost, c->stream));
    HIPCHK (hipEventRecord (q->look_ev[slot], c->stream));
    q->look_used[slot] = true; q->look_pushed[slot] = q->pushed;
  }
  q->n_push++;
  q->text_since = flush ? q->carry_bound : q->text_since + n_bytes;
  q->stream_bound = flush ? 0 : bound;
  if (flush && (rc = tjamd_scan_device (c, q->stream.p, need, q->m))) return rc;
  return TJAMD_OK;
}

extern "C" int tjamd_fastq_push_device (tjamd_counter *c, const void *d_text, size_t n_bytes, int final)
{
  static const char *fn = "tjamd_fastq_push_device";
  int rc = fastq_enter (fn, c, d_text, n_bytes, true, 0);
  if (rc) return rc;
  FastqSession *q = c->fq;
  if (!q || !q->open) return set_err (TJAMD_ERR_ARG, "%s: TJAMD_ERR_ARG: no session is open on this counter (tjamd_fastq_begin opens one)", fn);
  if (q->final_seen) return set_err (TJAMD_ERR_ARG, "%s: TJAMD_ERR_ARG: a push behind the final one", fn);
  rc = fastq_push (c, d_text, n_bytes, final, false);
  if (!rc && final) q->final_seen = true;
  return rc;
}

extern "C" int tjamd_fastq_push_host (tjamd_counter *c, const void *h_text, size_t n_bytes, int final)
{
  static const char *fn = "tjamd_fastq_push_host";
  int rc = fastq_enter (fn, c, h_text, n_bytes, false, 0);
  if (rc) return rc;
  FastqSession *q = c->fq;
  if (!q || !q->open) return set_err (TJAMD_ERR_ARG, "%s: TJAMD_ERR_ARG: no session is open on this counter (tjamd_fastq_begin opens one)", fn);
  if (q->final_seen) return set_err (TJAMD_ERR_ARG, "%s: TJAMD_ERR_ARG: a push behind the final one", fn);
  if (n_bytes) {
    rc = ensure (q->text, ((n_bytes + 15) & ~(size_t) 15) + 256, c->stream);
    if (rc) return rc;
    hipPointerAttribute_t at;
    const bool pinned = hipPointerGetAttributes (&at, h_text) == hipSuccess && at.type == hipMemoryTypeHost;
    (void) hipGetLastError ();                          // (pageable memory is an error to that call, not to this one)
    if (pinned) HIPCHK (hipMemcpyAsync (q->text.p, h_text, n_bytes, hipMemcpyHostToDevice, c->stream));
    else {
      for (size_t at_byte = 0; at_byte < n_bytes; at_byte += FQ_STAGE_BYTES) {
        const int b = q->pin_next;
        const size_t part = std::min ((size_t) FQ_STAGE_BYTES, n_bytes - at_byte);
        if (!q->pin[b]) { HIPCHK (hipHostMalloc (&q->pin[b], FQ_STAGE_BYTES, hipHostMallocDefault)); HIPCHK (hipEventCreateWithFlags (&q->pin_ev[b], hipEventDisableTiming)); }
        if (q->pin_used[b]) HIPCHK (hipEventSynchronize (q->pin_ev[b]));   // (the one wait of a push: this buffer's copy of two parts ago)
        memcpy (q->pin[b], (const char *) h_text + at_byte, part);
        HIPCHK (hipMemcpyAsync ((char *) q->text.p + at_byte, q->pin[b], part, hipMemcpyHostToDevice, c->stream));
        HIPCHK (hipEventRecord (q->pin_ev[b], c->stream));
        q->pin_used[b] = true; q->pin_next = b ^ 1;
      }
    }
  }
  return tjamd_fastq_push_device (c, n_bytes ? q->text.p : nullptr, n_bytes, final);
}

extern "C" long tjamd_fastq_end (tjamd_counter *c)
{
  static const char *fn = "tjamd_fastq_end";
  int rc = fastq_enter (fn, c, nullptr, 0, false, 0);
  if (rc) return -rc;
  FastqSession *q = c->fq;
  if (!q || !q->open) return -set_err (TJAMD_ERR_ARG, "%s: TJAMD_ERR_ARG: no session is open on this counter", fn);
  if (q->m >= 0 && q->stream_bound > 0 && (rc = fastq_push (c, nullptr, 0, 0, true))) return -rc;   // (the stream that has not gone to the scan yet)
  q->open = false;
  FqState h;
  static_assert (sizeof (FqState) % 4 == 0, "read back in words");
  rc = read_back (c, fn, q->state.p, &h, sizeof (FqState) / 4);
  if (rc) return -rc;
  q->consumed = (long) h.consumed; q->reads = (long) h.reads; q->stream_bytes = (long) h.stream_total;
  q->stop = h.stop ? (int) h.stop : (h.tail_len ? 1 : 0);
  q->kept = q->m < 0; q->ended = true;
  (void) __atomic_add_fetch (&g_fastq_sessions, 1, __ATOMIC_RELAXED);
  double ms = 0.0;
  for (long i = 0; i < q->n_push && i < FQ_TIMED_PUSHES; i++) { float f = 0.f; if (hipEventElapsedTime (&f, q->ev[2 * i], q->ev[2 * i + 1]) != hipSuccess) { ms = -1.0; break; } ms += (double) f; }
  q->ms = q->n_push > FQ_TIMED_PUSHES ? -1.0 : ms;
  (void) hipGetLastError ();
  return q->consumed;
}

extern "C" long tjamd_fastq_reads (const tjamd_counter *c) { return c && c->fq && c->fq->ended ? c->fq->reads : -1; }
extern "C" int tjamd_fastq_stop (const tjamd_counter *c) { return c && c->fq && c->fq->ended ? c->fq->stop : -1; }
extern "C" const void *tjamd_fastq_stream (const tjamd_counter *c) { return c && c->fq && c->fq->ended && c->fq->kept ? c->fq->stream.p : nullptr; }
extern "C" long tjamd_fastq_stream_bytes (const tjamd_counter *c) { return c && c->fq && c->fq->ended ? c->fq->stream_bytes : -1; }
extern "C" double tjamd_last_fastq_ms (tjamd_counter *c) { return c && c != g_fastq_refused && c->fq && c->fq->ended ? c->fq->ms : -1.0; }
