// The open-addressing table of voxel.hip (cell key -> lowest row, population) and voxel_reduce.hip ((segment, label) -> votes), in
// ONE place: 16-byte slots with a 64-bit key first, one table per cloud, a power of two of slots that is at least twice the cloud's
// rows.  Which slot a key lands in depends on who wins a compare-and-swap; the callers write out nothing that does.
#pragma once
#include <cstddef>
#include "pn2_common.h"

constexpr unsigned long long kEmpty = ~0ull;                        // no key: the callers' keys stay below 2^63

// Slots of a table for `rows` rows: the power of two >= 2 * rows, and >= 64.  ONE rule for the host's sizing (rows = max_rows) and
// for the capacity a kernel uses (rows = the cloud's device-side count, clamped to max_rows): it is monotone, so used <= allocated.
__host__ __device__ constexpr int64_t pn2_slot_capacity(int64_t rows) {
    return rows <= 32 ? 64 : (int64_t)1 << (64 - __builtin_clzll((unsigned long long)(2 * rows - 1)));
}
static_assert(pn2_slot_capacity(0) == 64 && pn2_slot_capacity(1) == 64 && pn2_slot_capacity(32) == 64 && pn2_slot_capacity(33) == 128,
              "64 slots up to 32 rows");
static_assert(pn2_slot_capacity(4095) == 8192 && pn2_slot_capacity(4096) == 8192 && pn2_slot_capacity(4097) == 16384,
              "2 * rows, rounded up to a power of two");
static_assert(pn2_slot_capacity(PN2_VOXEL_MAX_ROWS) == (int64_t)1 << 30 && PN2_VOXEL_MAX_ROWS == 1 << 29,
              "the largest table: slot numbers and probe counts fit 32 bits");

// the (B, max_rows) both users of the table accept
static inline bool pn2_slot_shape_ok(int B, int64_t max_rows) { return B >= 1 && B <= 65535 && max_rows >= 0 && max_rows <= PN2_VOXEL_MAX_ROWS; }

__device__ __forceinline__ unsigned pn2_slot_mix(unsigned long long k) {       // (murmur3's finaliser; the choice shows in no output)
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (unsigned)k;
}

// The slot of `key` in a table of mask + 1 slots, claiming an empty one if the key is new; -1 when the probe ran out.
// No thread ever waits for another: a slot that holds another key simply moves the probe on, and the loop is bounded by one pass
// over the table.  It cannot run out while the table holds at most as many keys as the cloud has rows: at least half of the
// slots stay empty.
template <class SlotT>
__device__ __forceinline__ int pn2_slot_claim(SlotT *__restrict__ table, unsigned mask, unsigned long long key) {
    static_assert(sizeof(SlotT) == 16 && alignof(SlotT) == 16 && offsetof(SlotT, key) == 0, "one slot is one 16-byte word, the key first");
    unsigned s = pn2_slot_mix(key) & mask;
    for (unsigned probe = 0; probe <= mask; ++probe) {
        const unsigned long long seen = atomicCAS(&table[s].key, kEmpty, key);
        if (seen == kEmpty || seen == key) return (int)s;
        s = (s + 1) & mask;
    }
    return -1;
}

// The slot that holds `key`, -1 when the table has none: a read-only probe for a LATER launch than the claims (the launch boundary
// orders it behind them).  It stops at the first empty slot -- a claimed key lies before the first empty slot of its probe sequence,
// nothing is ever removed -- and is bounded by one pass over the table.
template <class SlotT>
__device__ __forceinline__ int pn2_slot_find(const SlotT *__restrict__ table, unsigned mask, unsigned long long key) {
    static_assert(sizeof(SlotT) == 16 && alignof(SlotT) == 16 && offsetof(SlotT, key) == 0, "one slot is one 16-byte word, the key first");
    unsigned s = pn2_slot_mix(key) & mask;
    for (unsigned probe = 0; probe <= mask; ++probe) {
        const unsigned long long seen = table[s].key;
        if (seen == key) return (int)s;
        if (seen == kEmpty) return -1;
        s = (s + 1) & mask;
    }
    return -1;
}

// an empty slot with the caller's two payload words (the workspace arrives holding garbage)
__host__ __device__ inline uint4 pn2_slot_empty(unsigned word2, unsigned word3) { return make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, word2, word3); }

// grid-stride store of `pattern` to `slots` slots, by workgroups of kSlotThreads threads along the grid's x dimension
constexpr int kSlotThreads = 256;
__device__ __forceinline__ void pn2_slot_fill(uint4 *__restrict__ table, int64_t slots, uint4 pattern) {
    for (int64_t i = (int64_t)blockIdx.x * kSlotThreads + threadIdx.x; i < slots; i += (int64_t)gridDim.x * kSlotThreads) table[i] = pattern;
}

// workgroups of kSlotThreads threads for one thread per item (a grid is never empty), and for a grid-stride clear of `slots` slots
constexpr int64_t kSlotGridCap = 1 << 16;
static inline unsigned pn2_slot_blocks(int64_t items) { return (unsigned)(items <= 0 ? 1 : pn2_cdiv(items, kSlotThreads)); }
static inline unsigned pn2_slot_clear_blocks(int64_t slots) {      // (capped before it is narrowed: voxel.hip clears B tables in one grid)
    const int64_t blocks = slots <= 0 ? 1 : pn2_cdiv(slots, kSlotThreads);
    return (unsigned)(blocks < kSlotGridCap ? blocks : kSlotGridCap);
}

namespace {

__global__ __launch_bounds__(kSlotThreads) void pn2_slot_clear_kernel(uint4 *__restrict__ table, int64_t slots, uint4 pattern) {
    pn2_slot_fill(table, slots, pattern);
}

}  // namespace
