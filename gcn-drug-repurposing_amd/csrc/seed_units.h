// seed_units.h -- the contract of a table of units, nodes[u * max_size .. + sizes[u]) strictly ascending node indices of one CSR network,
// stated once for the ops that take one (set_modules.hip, diamond.hip, seed_connect.hip): what makes a unit bad, how a kernel finds that
// before it reads a row of the unit, and the words the host refuses the call with.  Device and host code.
//
// A kernel opens every unit with unit_size, ORs unit_member_bits over the unit's entries (and unit_row_bits over the CSR's rows where
// the op states a max_deg) and closes with unit_refused: a bad unit is skipped by its whole workgroup and leaves its bits in the call's
// status word.  The entry point holds a UnitStatus around the launch: begin() clears the word, end() turns it into the refusal.
#pragma once
#include "device_scope.h"

namespace gss {
namespace {   // as device_scope.h: every file that includes this has its own copy and the library exports nothing from here

// The bits of the status word.  UnitStatus::end reports the lowest one set.
constexpr int kUnitSize = 1;             // a unit's size is outside [0, max_size]
constexpr int kUnitNode = 2;             // an entry of a unit is outside [0, n)
constexpr int kUnitOrder = 4;            // an entry that is a node is not above its predecessor
constexpr int kUnitRow = 8;              // a row of the CSR is longer than the max_deg the caller states (or of negative length)

// sizes[u] when unit u may be walked, else a negative value with kUnitSize set: the same word for every thread, so the whole workgroup
// moves on.  (A negative size is returned as it is and only the too large one replaced: the caller's test is then on the loaded word, and
// diamond.hip, which has no register to spare, keeps its allocation.)
__device__ __forceinline__ int32_t unit_size(const int32_t *sizes, int64_t u, int32_t max_size, int32_t *flag) {
  const int32_t m = sizes[u];
  if ((m < 0 || m > max_size) && threadIdx.x == 0) atomicOr(flag, kUnitSize);
  return m > max_size ? -1 : m;
}

// the bits of entry i of the unit x[0 .. m)
__device__ __forceinline__ int unit_member_bits(const int32_t *x, int32_t i, int32_t n) {
  const int32_t v = x[i];
  if (v < 0 || v >= n) return kUnitNode;
  return i > 0 && x[i - 1] >= v ? kUnitOrder : 0;
}

// the bit of row v of the CSR
__device__ __forceinline__ int unit_row_bits(const int32_t *rowptr, int32_t v, int32_t max_deg) {
  const int32_t deg = rowptr[v + 1] - rowptr[v];
  return deg < 0 || deg > max_deg ? kUnitRow : 0;
}

// The verdict on a unit, from every thread's bits: nonzero, the same for every thread, when the unit is refused.  A barrier.
__device__ __forceinline__ int unit_refused(int bad, int32_t *flag) {
  if (bad) atomicOr(flag, bad);
  return __syncthreads_or(bad);
}

// The status word of one call.  `who` is the entry point's name in its refusals, `noun` what it calls an entry ("member", "seed").
struct UnitStatus {
  DeviceBuf<int32_t> flag;
  int begin(const char *who, hipStream_t st) {
    if (int rc = flag.alloc(who, sizeof(int32_t))) return rc;
    GSS_HIP(hipMemsetAsync(flag.p, 0, sizeof(int32_t), st));
    return GSS_OK;
  }
  // after the launch: waits for the stream.  An op that sets no kUnitRow passes any max_deg
  int end(const char *who, const char *noun, int32_t n, int32_t max_size, int32_t max_deg, hipStream_t st) {
    int32_t h = 0;
    if (int rc = read_back(&h, flag.p, sizeof(int32_t), st)) return rc;
    GSS_REQUIRE(!(h & kUnitSize), "%s: a unit's size is outside [0, max_size=%d]", who, max_size);
    GSS_REQUIRE(!(h & kUnitNode), "%s: a %s is not a node index in [0, %d)", who, noun, n);
    GSS_REQUIRE(!(h & kUnitOrder), "%s: a unit's %ss are not strictly ascending", who, noun);
    GSS_REQUIRE(!(h & kUnitRow), "%s: a row of the CSR is longer than max_deg=%d", who, max_deg);
    return GSS_OK;
  }
};

}  // namespace
}  // namespace gss
