// enc_dev.h — device helpers shared by the wire encoders (w2_encode.hip,
// w1_issue.hip, w1_reply.hip, result_encode.hip): short header runs gathered into dword stores
// (Put), payload copies by aligned 16-byte destination chunks (copy_chunk,
// copy_run) and the end of a size kernel (enc_place).
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

namespace mochi {

// ---- short byte runs --------------------------------------------------------
// A lane's header bytes lie in runs of ~30 between the payloads it skips.  The
// bytes are gathered into the aligned dword they fall in and go out as one
// dword store once the lane has written all four; the partial dword at either
// end of a run (its other bytes are payload or another lane's header) is
// written with byte stores.  ~3x fewer scattered stores than byte by byte.
struct Put {
  uint8_t* p;      // address of the next byte
  uint32_t w = 0;  // bytes gathered for the dword that holds p - 1
  uint32_t n = 0;  // how many (they end at p)
  __device__ __forceinline__ explicit Put(uint8_t* at) : p(at) {}
  __device__ __forceinline__ void flush() {
    if (n == 4) {
      *(uint32_t*)(p - 4) = w;  // n == 4 only when p is dword-aligned (byte())
    } else {
      const uint32_t sh = 8 * (uint32_t)((uintptr_t)(p - n) & 3);
#pragma unroll 1
      for (uint32_t k = 0; k < n; k++) (p - n)[k] = (uint8_t)(w >> (sh + 8 * k));
    }
    w = 0;
    n = 0;
  }
  __device__ __forceinline__ void byte(uint32_t b) {
    w |= (b & 0xFFu) << (8 * (uint32_t)((uintptr_t)p & 3));
    p++;
    n++;
    if (((uintptr_t)p & 3) == 0) flush();  // the dword is complete (n == 4) or its head was not ours (n < 4)
  }
  // leave a payload of `len` bytes to k_enc_copy
  __device__ __forceinline__ void skip(uint32_t len) {
    flush();
    p += len;
  }
  __device__ __forceinline__ void varint(uint64_t v) {
#pragma unroll 1
    while (v >= 0x80) {
      byte((uint32_t)v | 0x80);
      v >>= 7;
    }
    byte((uint32_t)v);
  }
  // The source is read as the aligned words that hold it, four independent
  // loads at a time (a word is loaded only if it holds a byte of the run, as
  // ByteReader's): a quarter of the load instructions of a byte-wise copy and
  // one load latency per 16 bytes (ids and keys are 10-30 bytes).
  __device__ __forceinline__ void bytes(const uint8_t* __restrict__ q, uint32_t len) {
    if (!len) return;
    const uintptr_t a = (uintptr_t)q;
    const uint32_t* wp = (const uint32_t*)(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3), nw = (sh + len + 3) >> 2;
#pragma unroll 1
    for (uint32_t w0 = 0; w0 < nw; w0 += 4) {
      uint32_t t[4];
#pragma unroll
      for (int j = 0; j < 4; j++) t[j] = w0 + j < nw ? wp[w0 + j] : 0u;
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
          const uint32_t idx = 4 * (w0 + j) + b;  // byte index counted from wp
          if (idx >= sh && idx < sh + len) byte(t[j] >> (8 * b));
        }
    }
  }
  __device__ __forceinline__ void ld(uint32_t tag, const uint8_t* __restrict__ q, uint32_t len) {
    byte(tag);
    varint(len);
    bytes(q, len);
  }
};

// ---- payload copy -----------------------------------------------------------
// 16-byte-aligned destination chunks holding a byte of the run [d0, d0 + len)
__device__ __forceinline__ uint32_t run_chunks(uintptr_t d0, uint32_t len) {
  return len ? (uint32_t)(((d0 + len - 1) >> 4) - (d0 >> 4)) + 1 : 0;
}

// Destination chunk c of the run src[0, len) -> [d0, d0 + len).  The lane owns
// the aligned chunk and assembles its 16 bytes from the one or two aligned
// SOURCE chunks that hold them: a dword rotation (mask selects) plus a funnel
// shift, k_w2_sig's read-side trick.  A source chunk is loaded only when it
// holds a payload byte (in bounds, as ByteReader's words).  A chunk that is all
// payload goes out as one dwordx4; the first / last partial chunk of a run is
// written with byte and short stores only, because its other bytes belong to
// headers written by another lane or kernel (a read-modify-write would race).
__device__ __forceinline__ void copy_chunk(uintptr_t d0, const uint8_t* __restrict__ src, uint32_t len, uint32_t c) {
  const uintptr_t A = (d0 & ~(uintptr_t)15) + 16 * (uintptr_t)c, dend = d0 + len;
  const uint32_t lo = A < d0 ? (uint32_t)(d0 - A) : 0;
  const uint32_t hi = dend - A < 16 ? (uint32_t)(dend - A) : 16;
  const uintptr_t S = (uintptr_t)src + (A - d0);  // source address of the chunk's byte 0 (modular when A < d0)
  const uint4* cp = (const uint4*)(S & ~(uintptr_t)15);
  const uint32_t sh = (uint32_t)(S & 15);
  const uint4 z = make_uint4(0, 0, 0, 0);
  const uint4 c0 = lo < 16 - sh ? cp[0] : z;  // holds source bytes [lo, 16 - sh) of the chunk
  const uint4 c1 = sh + hi > 16 ? cp[1] : z;  // holds [16 - sh, hi)
  const uint32_t d[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  const uint32_t m4 = 0u - ((sh >> 2) & 1u), m8 = 0u - ((sh >> 3) & 1u);
  uint32_t e1[7], e[5];
#pragma unroll
  for (int j = 0; j < 7; j++) e1[j] = (d[j + 1] & m4) | (d[j] & ~m4);
#pragma unroll
  for (int j = 0; j < 5; j++) e[j] = (e1[j + 2] & m8) | (e1[j] & ~m8);
  const uint32_t r = 8 * (sh & 3);
  const uint4 v = make_uint4(__builtin_amdgcn_alignbit(e[1], e[0], r), __builtin_amdgcn_alignbit(e[2], e[1], r),
                             __builtin_amdgcn_alignbit(e[3], e[2], r), __builtin_amdgcn_alignbit(e[4], e[3], r));
  if (lo == 0 && hi == 16) {
    *(uint4*)A = v;
    return;
  }
#pragma unroll 1
  for (uint32_t i = lo; i < hi;) {
    const uint32_t w = (i < 4 ? v.x : i < 8 ? v.y : i < 12 ? v.z : v.w) >> (8 * (i & 3));
    if (!(i & 1) && i + 2 <= hi) {
      *(uint16_t*)(A + i) = (uint16_t)w;
      i += 2;
    } else {
      *(uint8_t*)(A + i) = (uint8_t)w;
      i++;
    }
  }
}

// 16 lanes share two runs (a grant and its signature, a key and its hash) as
// one list of chunks: lane l takes chunks l, l + 16, ... of the first run and
// goes on into the second with the chunk index it carried over.  copy_run is
// one run, from chunk c, and returns the index to start the next run with; an
// absent next run is the caller's early return before it forms that address.
__device__ __forceinline__ uint32_t copy_run(uint32_t c, uintptr_t d0, const uint8_t* src, uint32_t len) {
  const uint32_t n = run_chunks(d0, len);
#pragma unroll 1
  for (; c < n; c += 16) copy_chunk(d0, src, len, c);
  return c - n;
}

// ---- end of a size kernel ----------------------------------------------------
// Lane i of n + 1 has the length `mine` of message i (0 for i >= n).  kSmall
// (one block of 1024 lanes, n < 1024): the 64-bit exclusive scan runs in the
// block, msg_off[i] and the total off64[n] are final.  Otherwise len64[0, n] is
// the input of the device-wide scan that follows (enc_launch.h
// enc_scan_offsets).  EVERY lane of the block must call this, also the lanes
// past n: the block scan has barriers.
template <bool kSmall>
__device__ __forceinline__ void enc_place(uint32_t i, uint32_t n, uint64_t mine, uint64_t* __restrict__ len64,
                                          uint64_t* __restrict__ off64, uint64_t* __restrict__ msg_off) {
  if constexpr (kSmall) {
    using Scan = hipcub::BlockScan<uint64_t, 1024>;
    __shared__ typename Scan::TempStorage tmp;
    uint64_t off;
    Scan(tmp).ExclusiveSum(mine, off);
    if (i < n) msg_off[i] = off;
    if (i == n) off64[n] = off;
  } else {
    if (i <= n) len64[i] = mine;
  }
}

}  // namespace mochi
