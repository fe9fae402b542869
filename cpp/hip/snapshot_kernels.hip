// gfx950 (MI355X / CDNA4) kernels for the snapshot engine: dirty-page
// tracking, XOR delta, diff compaction and typed merge application over
// HBM3E-resident snapshots.
//
// These replace the reference's CPU byte-crunching loops
// (reference: src/util/snapshot.cpp:30 diffArrayRegions, :363-402
// applyDiff(s), util/snapshot.h:163-246 calculateDiffValue/applyDiffValue,
// src/util/dirty.cpp trackers — fault-driven tracking has no HBM
// equivalent, so dirty pages come from a compare kernel against the
// baseline, the reference's DIFFING_MODE=xor made native).
//
// Design notes (per /opt/skills/guides/cdna_hip_programming.md):
//  - memory-bound throughout: 16 B/lane uint4 loads (G13), 256-thread
//    blocks. The page diff/apply kernels launch one wave per page with
//    NO grid cap: a 2048-block grid-stride form measured 4.87 TB/s at
//    25% scattered dirty vs 5.92 uncapped — the chip wants >>256
//    independent workgroups, not resident loops (G11 applies to the
//    small helper kernels only)
//  - one 4 KiB page = one 256-thread block iteration (256 × 16 B);
//    per-wave ballot keeps dirty-flag atomics to ≤4 per dirty page (G12)
//  - compaction via device-scope atomic ticket per dirty page; payload
//    writes stay coalesced within the page

#include <hip/hip_runtime.h>

#include <cstdint>

#define FAM_KERNEL_BLOCK 256
#define FAM_MAX_BLOCKS 2048
#define FAM_PAGE 4096

namespace {

using u8 = uint8_t;
using u32 = uint32_t;
using u64 = uint64_t;

__device__ __forceinline__ bool neq16(const uint4& a, const uint4& b)
{
    return (a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w);
}

// ---------------------------------------------------------------------------
// Dirty-page bitmap: flags[p] = 1 where any byte of 4 KiB page p differs.
// Each block iteration covers one page: 256 lanes × 16 B.
// ---------------------------------------------------------------------------
typedef unsigned int nt_u32v4 __attribute__((ext_vector_type(4)));

template<bool NT>
__device__ inline uint4 ldVec(const uint4* p)
{
    if constexpr (NT) {
        nt_u32v4 v =
          __builtin_nontemporal_load((const nt_u32v4*)p);
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    return *p;
}

template<bool NT>
__device__ inline void stVec(uint4* p, uint4 v)
{
    if constexpr (NT) {
        nt_u32v4 w = { v.x, v.y, v.z, v.w };
        __builtin_nontemporal_store(w, (nt_u32v4*)p);
    } else {
        *p = v;
    }
}

__global__ __launch_bounds__(FAM_KERNEL_BLOCK) void dirtyPagesKernel(
  const uint4* __restrict__ snap,
  const uint4* __restrict__ cur,
  u32 nPages,
  u32* __restrict__ flags)
{
    const u32 vecsPerPage = FAM_PAGE / 16; // 256
    for (u32 page = blockIdx.x; page < nPages; page += gridDim.x) {
        u64 v = (u64)page * vecsPerPage + threadIdx.x;
        bool diff = neq16(ldVec<true>(&snap[v]), ldVec<true>(&cur[v]));
        u64 mask = __ballot(diff);
        if ((threadIdx.x & 63) == 0 && mask != 0) {
            atomicOr(&flags[page], 1u);
        }
    }
}

// ---------------------------------------------------------------------------
// XOR delta over a whole buffer: out = a ^ b (16 B/lane, grid-stride)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(FAM_KERNEL_BLOCK) void xorBufferKernel(
  const uint4* __restrict__ a,
  const uint4* __restrict__ b,
  uint4* __restrict__ out,
  u64 nVec)
{
    // 2-way unrolled like copyBufferKernel: overlaps the second pair of
    // loads with the first store's drain
    u64 stride = (u64)gridDim.x * blockDim.x;
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + stride < nVec; i += 2 * stride) {
        uint4 x0 = ldVec<true>(&a[i]);
        uint4 y0 = ldVec<true>(&b[i]);
        uint4 x1 = ldVec<true>(&a[i + stride]);
        uint4 y1 = ldVec<true>(&b[i + stride]);
        stVec<true>(&out[i], make_uint4(x0.x ^ y0.x, x0.y ^ y0.y,
                                        x0.z ^ y0.z, x0.w ^ y0.w));
        stVec<true>(&out[i + stride],
                    make_uint4(x1.x ^ y1.x, x1.y ^ y1.y, x1.z ^ y1.z,
                               x1.w ^ y1.w));
    }
    for (; i < nVec; i += stride) {
        uint4 x = ldVec<true>(&a[i]);
        uint4 y = ldVec<true>(&b[i]);
        stVec<true>(&out[i],
                    make_uint4(x.x ^ y.x, x.y ^ y.y, x.z ^ y.z, x.w ^ y.w));
    }
}

// Plain device-to-device copy, nontemporal both sides: hipMemcpy D2D
// measures ~1.9 TB/s on MI355X while a grid-strided NT copy approaches
// the 2-unit HBM bound (~3.15 TB/s) — used for the single-rank
// collective short-circuits (MpiWorld)
__global__ __launch_bounds__(FAM_KERNEL_BLOCK) void copyBufferKernel(
  const uint4* __restrict__ src,
  uint4* __restrict__ dst,
  u64 nVec)
{
    // 2 vecs per lane per iteration: the second load issues while the
    // first store's cacheline drains
    u64 stride = (u64)gridDim.x * blockDim.x;
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + stride < nVec; i += 2 * stride) {
        uint4 a = ldVec<true>(&src[i]);
        uint4 b = ldVec<true>(&src[i + stride]);
        stVec<true>(&dst[i], a);
        stVec<true>(&dst[i + stride], b);
    }
    for (; i < nVec; i += stride) {
        stVec<true>(&dst[i], ldVec<true>(&src[i]));
    }
}

// ---------------------------------------------------------------------------
// Page diff, two-kernel pipeline:
//
//  (A) diffXorPagesKernel — one WAVE per page (64 lanes × 4 × 16 B = 4 KiB):
//      compare, and for dirty pages write the XOR payload SPARSELY at the
//      page's own slot plus one bit in a page bitmap. The bitmap atomics
//      are distributed over nPages/32 words, so there is no contention —
//      a single global ticket counter measured 1.07 TB/s at 100% dirty
//      (≈11 ns/atomic on one word, the "dequeue" price), the bitmap form
//      removes that serialization entirely.
//  (B) compactPageIdxKernel — scan the bitmap (2048 pages per wave
//      iteration) and emit the compacted dirty-page index list with ONE
//      ticket atomic per wave-iteration.
//
// Consumers (apply / ship) address the payload via pageIdx[slot] → page.
// ---------------------------------------------------------------------------
// The 4 GiB-scale working sets never fit in L2 (32 MiB/XCD), so the NT
// instantiation streams through with slc-tagged loads/stores
template<bool NT>
__global__ __launch_bounds__(FAM_KERNEL_BLOCK) void diffXorPagesKernel(
  const uint4* __restrict__ snap,
  const uint4* __restrict__ cur,
  u32 nPages,
  u32* __restrict__ bitmap, // nPages/32 words, zeroed before launch
  uint4* __restrict__ payloadOut) // sparse: indexed by page
{
    const u32 lane = threadIdx.x & 63;
    const u32 waveId =
      (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const u32 nWaves = (gridDim.x * blockDim.x) >> 6;
    const u32 vecsPerPage = FAM_PAGE / 16; // 256

    for (u32 page = waveId; page < nPages; page += nWaves) {
        u64 base = (u64)page * vecsPerPage + lane;
        uint4 s0 = ldVec<NT>(&snap[base]);
        uint4 s1 = ldVec<NT>(&snap[base + 64]);
        uint4 s2 = ldVec<NT>(&snap[base + 128]);
        uint4 s3 = ldVec<NT>(&snap[base + 192]);
        uint4 c0 = ldVec<NT>(&cur[base]);
        uint4 c1 = ldVec<NT>(&cur[base + 64]);
        uint4 c2 = ldVec<NT>(&cur[base + 128]);
        uint4 c3 = ldVec<NT>(&cur[base + 192]);
        bool diff = neq16(s0, c0) || neq16(s1, c1) || neq16(s2, c2) ||
                    neq16(s3, c3);
        u64 mask = __ballot(diff);
        if (mask == 0) {
            continue;
        }
        if (lane == 0) {
            atomicOr(&bitmap[page >> 5], 1u << (page & 31));
        }
        stVec<NT>(&payloadOut[base],
          make_uint4(s0.x ^ c0.x, s0.y ^ c0.y, s0.z ^ c0.z, s0.w ^ c0.w));
        stVec<NT>(&payloadOut[base + 64],
          make_uint4(s1.x ^ c1.x, s1.y ^ c1.y, s1.z ^ c1.z, s1.w ^ c1.w));
        stVec<NT>(&payloadOut[base + 128],
          make_uint4(s2.x ^ c2.x, s2.y ^ c2.y, s2.z ^ c2.z, s2.w ^ c2.w));
        stVec<NT>(&payloadOut[base + 192],
          make_uint4(s3.x ^ c3.x, s3.y ^ c3.y, s3.z ^ c3.z, s3.w ^ c3.w));
    }
}

// Compact the dirty-page bitmap into an index list. Each wave sweeps 64
// words (2048 pages) per iteration and takes a single base ticket.
__global__ __launch_bounds__(FAM_KERNEL_BLOCK) void compactPageIdxKernel(
  const u32* __restrict__ bitmap,
  u32 nWords,
  u32* __restrict__ ticket,
  u32* __restrict__ pageIdxOut)
{
    const u32 lane = threadIdx.x & 63;
    const u32 waveId =
      (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const u32 nWaves = (gridDim.x * blockDim.x) >> 6;

    for (u32 w0 = waveId * 64; w0 < nWords; w0 += nWaves * 64) {
        u32 word = (w0 + lane) < nWords ? bitmap[w0 + lane] : 0u;
        u32 mine = __popc(word);
        // Hillis-Steele inclusive scan over the wave's 64 lane counts
        u32 scan = mine;
        for (u32 off = 1; off < 64; off <<= 1) {
            u32 up = (u32)__shfl_up((int)scan, (int)off);
            if (lane >= off) {
                scan += up;
            }
        }
        u32 prefix = scan - mine; // exclusive
        u32 waveTotal = (u32)__shfl((int)scan, 63);
        if (waveTotal == 0) {
            continue;
        }
        u32 base = 0;
        if (lane == 63) {
            base = atomicAdd(ticket, waveTotal);
        }
        base = (u32)__shfl((int)base, 63);
        u32 out = base + prefix;
        u32 pageBase = (w0 + lane) * 32;
        while (word != 0) {
            u32 bit = __ffs(word) - 1;
            pageIdxOut[out++] = pageBase + bit;
            word &= word - 1;
        }
    }
}

// ---------------------------------------------------------------------------
// Apply XOR page diffs: snap[page] ^= payload[...] for page in pageIdx.
// One wave per dirty page. compact=0: payload is sparse (indexed by
// page, the diff kernel's output); compact=1: payload is slot-compacted
// (the shippable wire form).
// ---------------------------------------------------------------------------
template<bool NT>
__global__ __launch_bounds__(FAM_KERNEL_BLOCK) void applyXorPagesKernel(
  uint4* __restrict__ snap,
  const u32* __restrict__ pageIdx,
  const uint4* __restrict__ payload,
  u32 nDirty,
  int compact)
{
    const u32 lane = threadIdx.x & 63;
    const u32 waveId =
      (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const u32 nWaves = (gridDim.x * blockDim.x) >> 6;
    const u32 vecsPerPage = FAM_PAGE / 16;

    for (u32 slot = waveId; slot < nDirty; slot += nWaves) {
        u32 page = pageIdx[slot];
        u64 dst = (u64)page * vecsPerPage + lane;
        u64 src = compact ? (u64)slot * vecsPerPage + lane : dst;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint4 p = ldVec<NT>(&payload[src + k * 64]);
            uint4 s = ldVec<NT>(&snap[dst + k * 64]);
            stVec<NT>(&snap[dst + k * 64],
              make_uint4(s.x ^ p.x, s.y ^ p.y, s.z ^ p.z, s.w ^ p.w));
        }
    }
}

// Gather sparse per-page payloads into the compact wire form:
// out[slot] = payload[pageIdx[slot]]
__global__ __launch_bounds__(FAM_KERNEL_BLOCK) void gatherPagesKernel(
  const uint4* __restrict__ payload,
  const u32* __restrict__ pageIdx,
  uint4* __restrict__ out,
  u32 nDirty)
{
    const u32 lane = threadIdx.x & 63;
    const u32 waveId =
      (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const u32 nWaves = (gridDim.x * blockDim.x) >> 6;
    const u32 vecsPerPage = FAM_PAGE / 16;

    for (u32 slot = waveId; slot < nDirty; slot += nWaves) {
        u32 page = pageIdx[slot];
        u64 src = (u64)page * vecsPerPage + lane;
        u64 dst = (u64)slot * vecsPerPage + lane;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            stVec<true>(&out[dst + k * 64],
                        ldVec<true>(&payload[src + k * 64]));
        }
    }
}

// ---------------------------------------------------------------------------
// Typed elementwise merge: inout[i] = op(inout[i], in[i])
// (MPI op_reduce device form + snapshot typed merges; reference CPU loops
// src/mpi/MpiWorld.cpp:1266-1389, util/snapshot.h:216-246)
// ---------------------------------------------------------------------------
enum FamOp : int
{
    FAM_OP_SUM = 0,
    FAM_OP_MAX = 1,
    FAM_OP_MIN = 2,
    FAM_OP_PROD = 3,
    FAM_OP_SUB = 4,
    FAM_OP_XOR = 5,
};

template<typename T>
__device__ __forceinline__ T famApply(int op, T a, T b)
{
    switch (op) {
        case FAM_OP_SUM:
            return a + b;
        // Operand order of std::max/std::min(inout, in), as the host plane
        // (opReduceLoop): a NaN operand or a +0.0/-0.0 tie keeps `a`
        case FAM_OP_MAX:
            return a < b ? b : a;
        case FAM_OP_MIN:
            return b < a ? b : a;
        case FAM_OP_PROD:
            return a * b;
        case FAM_OP_SUB:
            return a - b;
    }
    return a;
}

template<typename T>
__global__ __launch_bounds__(FAM_KERNEL_BLOCK) void elementwiseOpKernel(
  T* __restrict__ inout,
  const T* __restrict__ in,
  u64 n,
  int op)
{
    // `in` is read once (NT); `inout` is RMW and keeps cached accesses
    // (same finding as the apply kernel: streaming the RMW side regresses)
    u64 stride = (u64)gridDim.x * blockDim.x;
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + stride < n; i += 2 * stride) {
        T a0 = __builtin_nontemporal_load(&in[i]);
        T a1 = __builtin_nontemporal_load(&in[i + stride]);
        inout[i] = famApply<T>(op, inout[i], a0);
        inout[i + stride] = famApply<T>(op, inout[i + stride], a1);
    }
    for (; i < n; i += stride) {
        inout[i] = famApply<T>(op, inout[i],
                               __builtin_nontemporal_load(&in[i]));
    }
}

__global__ __launch_bounds__(FAM_KERNEL_BLOCK) void xorBytesKernel(
  u8* __restrict__ inout,
  const u8* __restrict__ in,
  u64 n)
{
    // Unaligned-safe byte XOR for small typed diffs
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (u64)gridDim.x * blockDim.x) {
        inout[i] ^= in[i];
    }
}

__device__ inline u64 xorshift64(u64 x)
{
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    return x;
}

// Fill a buffer with deterministic pseudo-random bytes (bench init for
// the "random-byte region" snapshot shapes — BASELINE.json config 4)
__global__ __launch_bounds__(FAM_KERNEL_BLOCK) void fillRandomKernel(
  u64* __restrict__ out,
  u64 nWords,
  u64 seed)
{
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nWords;
         i += (u64)gridDim.x * blockDim.x) {
        out[i] = xorshift64(seed ^ (i * 0x9e3779b97f4a7c15ULL) ^
                            (i >> 3));
    }
}

// Mutate a scattered set of pages in place (wave per page, every lane
// perturbs its 64-byte slice) so the diff kernels face a randomized
// dirty distribution, not a contiguous memset
__global__ __launch_bounds__(FAM_KERNEL_BLOCK) void touchPagesKernel(
  u64* __restrict__ buf,
  const u32* __restrict__ pages,
  u32 nPages,
  u64 seed)
{
    const u32 wavesPerBlock = FAM_KERNEL_BLOCK / 64;
    const u32 wave = threadIdx.x / 64;
    const u32 lane = threadIdx.x % 64;
    const u32 wordsPerPage = FAM_PAGE / 8; // 512
    for (u32 p = blockIdx.x * wavesPerBlock + wave; p < nPages;
         p += gridDim.x * wavesPerBlock) {
        u64 base = (u64)pages[p] * wordsPerPage;
        for (u32 w = lane; w < wordsPerPage; w += 64) {
            buf[base + w] ^= xorshift64(seed ^ (base + w));
        }
    }
}

// ---------------------------------------------------------------------------
// State-KV mirror commit: scatter the listed 4 KiB pages of a pinned host
// mirror to the same offsets of the HBM value. One block per listed page,
// one 16 B load (over the host link) + one 16 B store per lane. `src` and
// `pageIdx` are device-visible pointers to pinned host memory, read in
// place. The value's last page may be partial and its tail need not be a
// multiple of 16 B: exactly min(4096, valueBytes - page*4096) bytes are
// copied, nothing past the value is read or written.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(FAM_KERNEL_BLOCK) void famKvCommitPagesKernel(
  const u8* __restrict__ src,
  u8* __restrict__ dst,
  const u32* __restrict__ pageIdx,
  u32 nPages,
  u64 valueBytes)
{
    u32 slot = blockIdx.x;
    if (slot >= nPages) {
        return;
    }
    u64 base = (u64)pageIdx[slot] * FAM_PAGE;
    if (base >= valueBytes) {
        return;
    }
    u64 left = valueBytes - base;
    u32 n = left < FAM_PAGE ? (u32)left : (u32)FAM_PAGE;
    u32 off = threadIdx.x * 16;
    if (off + 16 <= n) {
        *(uint4*)(dst + base + off) = *(const uint4*)(src + base + off);
    } else if (off < n) {
        // The one lane holding the value's sub-16 B tail
        for (u32 i = off; i < n; i++) {
            dst[base + i] = src[base + i];
        }
    }
}

// ---------------------------------------------------------------------------
// Typed merge regions (THREADS fork-join over a shared reduction variable):
//
//  typedDiffKernel<T> — one WAVE per 4 KiB-aligned chunk of the region.
//      An element is changed when !(orig == cur) as T (calcDiffValue in
//      cpp/src/snapshot.cpp: NaN always, +0.0 vs -0.0 never). The wave
//      counts its changed elements per lane, scans the counts as
//      compactPageIdxKernel does and takes ONE ticket per chunk (none when
//      nothing changed), then every lane writes its own run of
//      {element index, value} entries. The 16 B-aligned interior of the
//      chunk loads 16 B per lane (4 vectors per lane, as the page diff);
//      the region's head and tail elements up to the next 16 B boundary
//      take a scalar load in the low lanes.
//  applyTypedElemsKernel<T> — base[idx[i]] = op(base[idx[i]], val[i]), one
//      lane per entry, cached RMW. Diffs are applied one after another on
//      one stream and an index occurs once per diff: no atomics.
//
// op is a SnapshotMergeOperation code, dtype a SnapshotDataType code.
// ---------------------------------------------------------------------------
enum FamMergeOp : int
{
    FAM_MERGE_SUM = 1,
    FAM_MERGE_PRODUCT = 2,
    FAM_MERGE_SUBTRACT = 3,
    FAM_MERGE_MAX = 4,
    FAM_MERGE_MIN = 5,
};

template<typename T>
struct TypedUnsigned
{
    using type = T; // floats subtract as themselves
};
template<>
struct TypedUnsigned<int32_t>
{
    using type = u32;
};
template<>
struct TypedUnsigned<int64_t>
{
    using type = u64;
};

// 0 = unchanged, 1 = emit `out`, 2 = product diff with a zero original
template<typename T>
__device__ __forceinline__ int typedDiffValue(int op, T orig, T cur, T& out)
{
    using U = typename TypedUnsigned<T>::type;
    if (orig == cur) {
        return 0;
    }
    switch (op) {
        case FAM_MERGE_SUM:
            // Integers wrap (two's complement): subtract unsigned
            out = (T)((U)cur - (U)orig);
            return 1;
        case FAM_MERGE_SUBTRACT:
            out = (T)((U)orig - (U)cur);
            return 1;
        case FAM_MERGE_PRODUCT:
            if (orig == (T)0) {
                return 2;
            }
            out = cur / orig;
            return 1;
        default: // Max, Min ship the value
            out = cur;
            return 1;
    }
}

template<typename T>
__global__ __launch_bounds__(FAM_KERNEL_BLOCK) void typedDiffKernel(
  const u8* __restrict__ snap,
  const u8* __restrict__ cur,
  u64 regionStart, // bytes, multiple of sizeof(T)
  u64 regionEnd,   // bytes, regionStart + nElems * sizeof(T)
  int op,
  u32* __restrict__ ticket,
  u32* __restrict__ errWord,
  u32* __restrict__ idxOut,
  T* __restrict__ valOut)
{
    constexpr u32 E = 16 / sizeof(T); // elements per 16 B vector
    const u32 lane = threadIdx.x & 63;
    const u64 waveId = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;

    // This wave's chunk, clipped to the region (all wave-uniform)
    const u64 chunk = regionStart / FAM_PAGE + waveId;
    u64 lo = chunk * FAM_PAGE;
    u64 hi = lo + FAM_PAGE;
    lo = lo < regionStart ? regionStart : lo;
    hi = hi > regionEnd ? regionEnd : hi;
    if (lo >= hi) {
        return;
    }
    // Elements never straddle a 16 B boundary: regionStart is a multiple
    // of sizeof(T), which divides 16
    u64 alo = (lo + 15) & ~(u64)15;
    u64 ahi = hi & ~(u64)15;
    if (alo > hi) {
        alo = hi; // the whole clip lies inside one 16 B line
    }
    if (ahi < alo) {
        ahi = alo;
    }
    const u32 nHead = (u32)((alo - lo) / sizeof(T)); // < E
    const u32 nTail = (u32)((hi - ahi) / sizeof(T)); // < E
    const u32 nVec = (u32)((ahi - alo) / 16);        // <= 256

    // Interior: 4 vectors per lane, loads issued before any compare
    uint4 s[4];
    uint4 c[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        u32 v = lane + 64 * k;
        if (v < nVec) {
            s[k] = ldVec<true>((const uint4*)(snap + alo) + v);
            c[k] = ldVec<true>((const uint4*)(cur + alo) + v);
        } else {
            s[k] = make_uint4(0, 0, 0, 0);
            c[k] = s[k];
        }
    }
    // Head and tail: one scalar element in each of the low lanes
    T hs = (T)0, hc = (T)0, ts = (T)0, tc = (T)0;
    if (lane < nHead) {
        hs = *(const T*)(snap + lo + lane * sizeof(T));
        hc = *(const T*)(cur + lo + lane * sizeof(T));
    }
    if (lane < nTail) {
        ts = *(const T*)(snap + ahi + lane * sizeof(T));
        tc = *(const T*)(cur + ahi + lane * sizeof(T));
    }

    // Pass 1: which of this lane's elements emit an entry
    u32 emitMask = 0; // bit k*E+e interior, bit 16 head, bit 17 tail
    bool zeroOrig = false;
    T tmp = (T)0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        T sv[E];
        T cv[E];
        __builtin_memcpy(sv, &s[k], 16);
        __builtin_memcpy(cv, &c[k], 16);
#pragma unroll
        for (u32 e = 0; e < E; e++) {
            int r = typedDiffValue<T>(op, sv[e], cv[e], tmp);
            emitMask |= (r == 1 ? 1u : 0u) << (k * E + e);
            zeroOrig |= r == 2;
        }
    }
    {
        int r = typedDiffValue<T>(op, hs, hc, tmp);
        emitMask |= (r == 1 ? 1u : 0u) << 16;
        zeroOrig |= r == 2;
        r = typedDiffValue<T>(op, ts, tc, tmp);
        emitMask |= (r == 1 ? 1u : 0u) << 17;
        zeroOrig |= r == 2;
    }
    if (__ballot(zeroOrig) != 0 && lane == 0) {
        atomicOr(errWord, 1u);
    }

    // Wave scan of the per-lane counts, one ticket per chunk
    u32 mine = __popc(emitMask);
    u32 scan = mine;
    for (u32 off = 1; off < 64; off <<= 1) {
        u32 up = (u32)__shfl_up((int)scan, (int)off);
        if (lane >= off) {
            scan += up;
        }
    }
    u32 waveTotal = (u32)__shfl((int)scan, 63);
    if (waveTotal == 0) {
        return;
    }
    u32 base = 0;
    if (lane == 63) {
        base = atomicAdd(ticket, waveTotal);
    }
    base = (u32)__shfl((int)base, 63);
    u32 out = base + (scan - mine);

    // Pass 2: emit {index relative to the region start, value}
#pragma unroll
    for (int k = 0; k < 4; k++) {
        T sv[E];
        T cv[E];
        __builtin_memcpy(sv, &s[k], 16);
        __builtin_memcpy(cv, &c[k], 16);
        u64 vecByte = alo + (u64)(lane + 64 * k) * 16;
#pragma unroll
        for (u32 e = 0; e < E; e++) {
            if (emitMask & (1u << (k * E + e))) {
                typedDiffValue<T>(op, sv[e], cv[e], tmp);
                idxOut[out] =
                  (u32)((vecByte - regionStart) / sizeof(T)) + e;
                valOut[out] = tmp;
                out++;
            }
        }
    }
    if (emitMask & (1u << 16)) {
        typedDiffValue<T>(op, hs, hc, tmp);
        idxOut[out] = (u32)((lo - regionStart) / sizeof(T)) + lane;
        valOut[out] = tmp;
        out++;
    }
    if (emitMask & (1u << 17)) {
        typedDiffValue<T>(op, ts, tc, tmp);
        idxOut[out] = (u32)((ahi - regionStart) / sizeof(T)) + lane;
        valOut[out] = tmp;
        out++;
    }
}

template<typename T>
__global__ __launch_bounds__(FAM_KERNEL_BLOCK) void applyTypedElemsKernel(
  T* __restrict__ base,
  const u32* __restrict__ idx,
  const T* __restrict__ val,
  u32 count,
  int famOp)
{
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) {
        T* p = base + idx[i];
        *p = famApply<T>(famOp, *p, val[i]);
    }
}

// SnapshotMergeOperation code -> FamOp, -1 where there is no typed merge
inline int famOpForMerge(int op)
{
    switch (op) {
        case FAM_MERGE_SUM:
            return FAM_OP_SUM;
        case FAM_MERGE_PRODUCT:
            return FAM_OP_PROD;
        case FAM_MERGE_SUBTRACT:
            return FAM_OP_SUB;
        case FAM_MERGE_MAX:
            return FAM_OP_MAX;
        case FAM_MERGE_MIN:
            return FAM_OP_MIN;
    }
    return -1;
}

// SnapshotDataType code -> element size, 0 where the type has no merges
inline u32 typedElemSize(int dtype)
{
    switch (dtype) {
        case 2: // Int
        case 4: // Float
            return 4;
        case 3: // Long
        case 5: // Double
            return 8;
    }
    return 0;
}

inline u32 gridFor(u64 items)
{
    // One element per lane, uncapped: a 2048-block grid-stride copy
    // measured 5.53 TB/s vs 6.42 at one-per-lane on 256 MB (the chip
    // wants >>256 independent workgroups)
    u64 blocks = (items + FAM_KERNEL_BLOCK - 1) / FAM_KERNEL_BLOCK;
    if (blocks == 0) {
        blocks = 1;
    }
    if (blocks > 0xffffffffu) {
        blocks = 0xffffffffu;
    }
    return (u32)blocks;
}

} // namespace

// --------------------------- C API ------------------------------------------

extern "C" {

hipError_t famDirtyPages(const void* snap,
                         const void* cur,
                         uint64_t bytes,
                         uint32_t* flagsDev,
                         hipStream_t stream)
{
    if ((bytes % FAM_PAGE) != 0) {
        // A silently-floored tail would be missed dirty data
        return hipErrorInvalidValue;
    }
    uint32_t nPages = (uint32_t)(bytes / FAM_PAGE);
    uint32_t grid = nPages ? nPages : 1; // block per page, uncapped
    hipLaunchKernelGGL(dirtyPagesKernel,
                       dim3(grid),
                       dim3(FAM_KERNEL_BLOCK),
                       0,
                       stream,
                       (const uint4*)snap,
                       (const uint4*)cur,
                       nPages,
                       flagsDev);
    return hipGetLastError();
}

hipError_t famFillRandom(void* buf,
                         uint64_t bytes,
                         uint64_t seed,
                         hipStream_t stream)
{
    if ((bytes % 8) != 0) {
        return hipErrorInvalidValue;
    }
    u64 nWords = bytes / 8;
    hipLaunchKernelGGL(fillRandomKernel,
                       dim3(gridFor(nWords)),
                       dim3(FAM_KERNEL_BLOCK),
                       0,
                       stream,
                       (u64*)buf,
                       nWords,
                       seed);
    return hipGetLastError();
}

hipError_t famTouchPages(void* buf,
                         const uint32_t* pagesDev,
                         uint32_t nPages,
                         uint64_t seed,
                         hipStream_t stream)
{
    u32 wavesPerBlock = FAM_KERNEL_BLOCK / 64;
    u32 blocks = (nPages + wavesPerBlock - 1) / wavesPerBlock;
    u32 grid = blocks < FAM_MAX_BLOCKS ? (blocks ? blocks : 1)
                                       : FAM_MAX_BLOCKS;
    hipLaunchKernelGGL(touchPagesKernel,
                       dim3(grid),
                       dim3(FAM_KERNEL_BLOCK),
                       0,
                       stream,
                       (u64*)buf,
                       pagesDev,
                       nPages,
                       seed);
    return hipGetLastError();
}

hipError_t famCopyBuffer(const void* src,
                         void* dst,
                         uint64_t bytes,
                         hipStream_t stream)
{
    if ((bytes % 16) != 0 ||
        (((uintptr_t)src | (uintptr_t)dst) & 15) != 0) {
        // Tail or base not vectorisable (callers pass user pointers, e.g.
        // a tensor view at a 4 B offset): fall back to the runtime copy
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice,
                              stream);
    }
    uint64_t nVec = bytes / 16;
    static const u32 copyGrid = []() {
        const char* e = getenv("FAM_COPY_GRID");
        return e ? (u32)atoi(e) : 0;
    }();
    u32 grid = copyGrid ? copyGrid : gridFor(nVec);
    if ((u64)grid * FAM_KERNEL_BLOCK > nVec && nVec > 0) {
        grid = gridFor(nVec);
    }
    hipLaunchKernelGGL(copyBufferKernel,
                       dim3(grid),
                       dim3(FAM_KERNEL_BLOCK),
                       0,
                       stream,
                       (const uint4*)src,
                       (uint4*)dst,
                       nVec);
    return hipGetLastError();
}

hipError_t famXorBuffer(const void* a,
                        const void* b,
                        void* out,
                        uint64_t bytes,
                        hipStream_t stream)
{
    if ((bytes % 16) != 0) {
        // No scalar tail path: reject rather than silently drop bytes
        return hipErrorInvalidValue;
    }
    uint64_t nVec = bytes / 16;
    hipLaunchKernelGGL(xorBufferKernel,
                       dim3(gridFor(nVec)),
                       dim3(FAM_KERNEL_BLOCK),
                       0,
                       stream,
                       (const uint4*)a,
                       (const uint4*)b,
                       (uint4*)out,
                       nVec);
    return hipGetLastError();
}

hipError_t famDiffXorPages(const void* snap,
                           const void* cur,
                           uint64_t bytes,
                           uint32_t* ticketDev, // one u32, zeroed by caller
                           uint32_t* pageIdxDev,
                           void* payloadDev,
                           uint32_t* bitmapDev, // nPages/32 words, zeroed
                           hipStream_t stream)
{
    if ((bytes % FAM_PAGE) != 0) {
        return hipErrorInvalidValue;
    }
    uint32_t nPages = (uint32_t)(bytes / FAM_PAGE);
    uint32_t wavesPerBlock = FAM_KERNEL_BLOCK / 64;
    uint32_t blocks = (nPages + wavesPerBlock - 1) / wavesPerBlock;
    // Launch one wave per page with NO grid cap by default: the old
    // 2048-block grid-stride form measured 4.87 TB/s at 25% scattered
    // dirty vs 5.92 uncapped on the same box (the stride loop starves
    // the 256-CU/8-XCD chip of independent blocks)
    static const uint32_t maxBlocks = []() {
        const char* e = getenv("FAM_DIFF_BLOCKS");
        uint32_t v = e ? (uint32_t)atoi(e) : 0;
        return v ? v : 0xffffffffu;
    }();
    uint32_t grid = blocks < maxBlocks ? (blocks ? blocks : 1)
                                       : maxBlocks;
    static const bool useNt = []() {
        const char* e = getenv("FAM_DIFF_NT");
        return e == nullptr || e[0] != '0'; // default on
    }();
    if (useNt) {
        hipLaunchKernelGGL(diffXorPagesKernel<true>,
                           dim3(grid),
                           dim3(FAM_KERNEL_BLOCK),
                           0,
                           stream,
                           (const uint4*)snap,
                           (const uint4*)cur,
                           nPages,
                           bitmapDev,
                           (uint4*)payloadDev);
    } else {
        hipLaunchKernelGGL(diffXorPagesKernel<false>,
                           dim3(grid),
                           dim3(FAM_KERNEL_BLOCK),
                           0,
                           stream,
                           (const uint4*)snap,
                           (const uint4*)cur,
                           nPages,
                           bitmapDev,
                           (uint4*)payloadDev);
    }
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        return err;
    }
    uint32_t nWords = (nPages + 31) / 32;
    uint32_t sweepWaves = (nWords + 63) / 64;
    uint32_t sweepBlocks = (sweepWaves + wavesPerBlock - 1) / wavesPerBlock;
    if (sweepBlocks == 0) {
        sweepBlocks = 1;
    }
    if (sweepBlocks > FAM_MAX_BLOCKS) {
        sweepBlocks = FAM_MAX_BLOCKS;
    }
    hipLaunchKernelGGL(compactPageIdxKernel,
                       dim3(sweepBlocks),
                       dim3(FAM_KERNEL_BLOCK),
                       0,
                       stream,
                       bitmapDev,
                       nWords,
                       ticketDev,
                       pageIdxDev);
    return hipGetLastError();
}

hipError_t famApplyXorPagesEx(void* snap,
                              const uint32_t* pageIdxDev,
                              const void* payloadDev,
                              uint32_t nDirty,
                              int compact,
                              hipStream_t stream)
{
    uint32_t wavesPerBlock = FAM_KERNEL_BLOCK / 64;
    uint32_t blocks = (nDirty + wavesPerBlock - 1) / wavesPerBlock;
    // Uncapped like the diff kernel (see famDiffXorPages)
    static const uint32_t maxApplyBlocks = []() {
        const char* e = getenv("FAM_APPLY_BLOCKS");
        uint32_t v = e ? (uint32_t)atoi(e) : 0;
        return v ? v : 0xffffffffu;
    }();
    uint32_t grid = blocks < maxApplyBlocks ? (blocks ? blocks : 1)
                                            : maxApplyBlocks;
    // Unlike diff, apply is a read-modify-write of the same lines: the
    // store hits L2 brought in by the load, so streaming hurts (A/B on
    // MI355X: 5.15 vs 5.30 TB/s) — default off
    static const bool useNtApply = []() {
        const char* e = getenv("FAM_APPLY_NT");
        return e != nullptr && e[0] == '1';
    }();
    auto* kern =
      useNtApply ? applyXorPagesKernel<true> : applyXorPagesKernel<false>;
    hipLaunchKernelGGL(kern,
                       dim3(grid),
                       dim3(FAM_KERNEL_BLOCK),
                       0,
                       stream,
                       (uint4*)snap,
                       pageIdxDev,
                       (const uint4*)payloadDev,
                       nDirty,
                       compact);
    return hipGetLastError();
}

hipError_t famApplyXorPages(void* snap,
                            const uint32_t* pageIdxDev,
                            const void* payloadDev,
                            uint32_t nDirty,
                            hipStream_t stream)
{
    return famApplyXorPagesEx(snap, pageIdxDev, payloadDev, nDirty, 0,
                              stream);
}

hipError_t famGatherPages(const void* payloadDev,
                          const uint32_t* pageIdxDev,
                          void* outDev,
                          uint32_t nDirty,
                          hipStream_t stream)
{
    uint32_t wavesPerBlock = FAM_KERNEL_BLOCK / 64;
    uint32_t blocks = (nDirty + wavesPerBlock - 1) / wavesPerBlock;
    // Uncapped like the diff kernel (see famDiffXorPages)
    static const uint32_t maxApplyBlocks = []() {
        const char* e = getenv("FAM_APPLY_BLOCKS");
        uint32_t v = e ? (uint32_t)atoi(e) : 0;
        return v ? v : 0xffffffffu;
    }();
    uint32_t grid = blocks < maxApplyBlocks ? (blocks ? blocks : 1)
                                            : maxApplyBlocks;
    hipLaunchKernelGGL(gatherPagesKernel,
                       dim3(grid),
                       dim3(FAM_KERNEL_BLOCK),
                       0,
                       stream,
                       (const uint4*)payloadDev,
                       pageIdxDev,
                       (uint4*)outDev,
                       nDirty);
    return hipGetLastError();
}

hipError_t famCommitPages(const void* srcHostMapped,
                          void* dstDev,
                          const uint32_t* pageIdx,
                          uint32_t nPages,
                          uint64_t valueBytes,
                          hipStream_t stream)
{
    if (nPages == 0) {
        return hipSuccess;
    }
    // Page offsets keep the 16 B lane accesses aligned only from
    // 16 B-aligned bases
    if ((((uintptr_t)srcHostMapped | (uintptr_t)dstDev) & 15) != 0) {
        return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(famKvCommitPagesKernel,
                       dim3(nPages),
                       dim3(FAM_KERNEL_BLOCK),
                       0,
                       stream,
                       (const u8*)srcHostMapped,
                       (u8*)dstDev,
                       pageIdx,
                       nPages,
                       valueBytes);
    return hipGetLastError();
}

// Typed diff with compaction of the region [regionStart, regionStart +
// nElems * sizeof(T)) of cur against snap. dtype is a SnapshotDataType
// code (Int, Long, Float, Double), op a SnapshotMergeOperation code (Sum,
// Product, Subtract, Max, Min). ticketDev and errDev are zeroed by the
// caller; after the stream drains *ticketDev is the entry count and
// *errDev is non-zero if a Product element had a zero original.
hipError_t famTypedDiff(const void* snap,
                        const void* cur,
                        uint64_t regionStart,
                        uint64_t nElems,
                        int dtype,
                        int op,
                        uint32_t* ticketDev,
                        uint32_t* errDev,
                        uint32_t* idxOutDev,
                        void* valOutDev,
                        hipStream_t stream)
{
    u32 elem = typedElemSize(dtype);
    if (elem == 0 || famOpForMerge(op) < 0 || (regionStart % elem) != 0 ||
        nElems > 0xffffffffull ||
        (((uintptr_t)snap | (uintptr_t)cur) & 15) != 0) {
        return hipErrorInvalidValue;
    }
    if (nElems == 0) {
        return hipSuccess;
    }
    u64 regionEnd = regionStart + nElems * elem;
    u64 nChunks = (regionEnd - 1) / FAM_PAGE - regionStart / FAM_PAGE + 1;
    u64 wavesPerBlock = FAM_KERNEL_BLOCK / 64;
    u64 blocks = (nChunks + wavesPerBlock - 1) / wavesPerBlock;
    // One wave per chunk, uncapped like the page diff (see famDiffXorPages)
    dim3 grid((u32)blocks);
    dim3 block(FAM_KERNEL_BLOCK);
    const u8* s = (const u8*)snap;
    const u8* c = (const u8*)cur;
    switch (dtype) {
        case 2:
            hipLaunchKernelGGL(typedDiffKernel<int32_t>,
                               grid, block, 0, stream,
                               s, c, regionStart, regionEnd, op, ticketDev,
                               errDev, idxOutDev, (int32_t*)valOutDev);
            break;
        case 3:
            hipLaunchKernelGGL(typedDiffKernel<int64_t>,
                               grid, block, 0, stream,
                               s, c, regionStart, regionEnd, op, ticketDev,
                               errDev, idxOutDev, (int64_t*)valOutDev);
            break;
        case 4:
            hipLaunchKernelGGL(typedDiffKernel<float>,
                               grid, block, 0, stream,
                               s, c, regionStart, regionEnd, op, ticketDev,
                               errDev, idxOutDev, (float*)valOutDev);
            break;
        default:
            hipLaunchKernelGGL(typedDiffKernel<double>,
                               grid, block, 0, stream,
                               s, c, regionStart, regionEnd, op, ticketDev,
                               errDev, idxOutDev, (double*)valOutDev);
    }
    return hipGetLastError();
}

// base[idx[i]] = op(base[idx[i]], val[i]) for i < count; base points at the
// region start and must be aligned to the element. The caller has checked
// every index against the allocation.
hipError_t famApplyTypedElems(void* base,
                              const uint32_t* idxDev,
                              const void* valDev,
                              uint32_t count,
                              int dtype,
                              int op,
                              hipStream_t stream)
{
    u32 elem = typedElemSize(dtype);
    int famOp = famOpForMerge(op);
    if (elem == 0 || famOp < 0 || ((uintptr_t)base % elem) != 0) {
        return hipErrorInvalidValue;
    }
    if (count == 0) {
        return hipSuccess;
    }
    dim3 grid(gridFor(count));
    dim3 block(FAM_KERNEL_BLOCK);
    switch (dtype) {
        case 2:
            hipLaunchKernelGGL(applyTypedElemsKernel<int32_t>,
                               grid, block, 0, stream,
                               (int32_t*)base, idxDev,
                               (const int32_t*)valDev, count, famOp);
            break;
        case 3:
            hipLaunchKernelGGL(applyTypedElemsKernel<int64_t>,
                               grid, block, 0, stream,
                               (int64_t*)base, idxDev,
                               (const int64_t*)valDev, count, famOp);
            break;
        case 4:
            hipLaunchKernelGGL(applyTypedElemsKernel<float>,
                               grid, block, 0, stream,
                               (float*)base, idxDev,
                               (const float*)valDev, count, famOp);
            break;
        default:
            hipLaunchKernelGGL(applyTypedElemsKernel<double>,
                               grid, block, 0, stream,
                               (double*)base, idxDev,
                               (const double*)valDev, count, famOp);
    }
    return hipGetLastError();
}

// dtype: 0=i32 1=i64 2=u64 3=f32 4=f64 5=byte (matches MpiDataType)
hipError_t famElementwiseOp(void* inout,
                            const void* in,
                            uint64_t count,
                            int dtype,
                            int op,
                            hipStream_t stream)
{
    // An unknown dtype or op, or XOR on a typed dtype, has no kernel: an
    // error, never a launch that writes every element back unchanged
    if (dtype < 0 || dtype > 5 || op < FAM_OP_SUM || op > FAM_OP_XOR ||
        (op == FAM_OP_XOR && dtype != 5)) {
        return hipErrorInvalidValue;
    }
    dim3 grid(gridFor(count));
    dim3 block(FAM_KERNEL_BLOCK);
    switch (dtype) {
        case 0:
            hipLaunchKernelGGL(elementwiseOpKernel<int32_t>,
                               grid, block, 0, stream,
                               (int32_t*)inout, (const int32_t*)in,
                               count, op);
            break;
        case 1:
            hipLaunchKernelGGL(elementwiseOpKernel<int64_t>,
                               grid, block, 0, stream,
                               (int64_t*)inout, (const int64_t*)in,
                               count, op);
            break;
        case 2:
            hipLaunchKernelGGL(elementwiseOpKernel<uint64_t>,
                               grid, block, 0, stream,
                               (uint64_t*)inout, (const uint64_t*)in,
                               count, op);
            break;
        case 3:
            hipLaunchKernelGGL(elementwiseOpKernel<float>,
                               grid, block, 0, stream,
                               (float*)inout, (const float*)in,
                               count, op);
            break;
        case 4:
            hipLaunchKernelGGL(elementwiseOpKernel<double>,
                               grid, block, 0, stream,
                               (double*)inout, (const double*)in,
                               count, op);
            break;
        default:
            if (op == FAM_OP_XOR) {
                hipLaunchKernelGGL(xorBytesKernel,
                                   grid, block, 0, stream,
                                   (u8*)inout, (const u8*)in, count);
            } else {
                hipLaunchKernelGGL(elementwiseOpKernel<u8>,
                                   grid, block, 0, stream,
                                   (u8*)inout, (const u8*)in, count, op);
            }
    }
    return hipGetLastError();
}

} // extern "C"
