// wide_tables.hpp — what the wide-letter kernels share (wide.hip's single
// stream encoder and long-code decoder, wdecode_ranges.hip, wbatch.hip): the
// letter types, the cuckoo code table of host/wide.hpp (WideEncTables) with its
// two-slot lookup, the lane's letters of a round, and the pieces of a 16-byte
// group of decoded letters.
#pragma once

#include <type_traits>

#include "bitreader.hpp"

namespace huff::dev {

struct U128 {
    uint64_t lo, hi;
};

// ---------------------------------------------------------------------------
// code table (host/wide.hpp wide_slot_layout)
template <uint32_t W>
using KeyT = std::conditional_t<(W <= 4), uint32_t, std::conditional_t<(W == 8), uint64_t, U128>>;

template <typename K, typename V>
struct Slot;
template <>
struct alignas(8) Slot<uint32_t, uint32_t> {
    uint32_t key, val;
};
template <>
struct alignas(16) Slot<uint32_t, uint64_t> {
    uint32_t key, pad;
    uint64_t val;
};
template <>
struct alignas(16) Slot<uint64_t, uint32_t> {
    uint64_t key;
    uint32_t val, pad;
};
template <>
struct alignas(16) Slot<uint64_t, uint64_t> {
    uint64_t key, val;
};
template <>
struct alignas(16) Slot<U128, uint32_t> {
    U128 key;
    uint32_t val, pad[3];
};
template <>
struct alignas(16) Slot<U128, uint64_t> {
    U128 key;
    uint64_t val, pad;
};
static_assert(sizeof(Slot<uint32_t, uint32_t>) == 8 && sizeof(Slot<uint32_t, uint64_t>) == 16 &&
                  sizeof(Slot<uint64_t, uint32_t>) == 16 && sizeof(Slot<U128, uint64_t>) == 32,
              "slots as host/wide.hpp wide_slot_layout");

__device__ __forceinline__ bool key_eq(uint32_t a, uint32_t b) { return a == b; }
__device__ __forceinline__ bool key_eq(uint64_t a, uint64_t b) { return a == b; }
__device__ __forceinline__ bool key_eq(U128 a, U128 b) { return a.lo == b.lo && a.hi == b.hi; }

// host/wide.hpp wide_hkey
template <uint32_t W>
__device__ __forceinline__ uint32_t hkey(KeyT<W> k, uint64_t fold) {
    if constexpr (W <= 4) {
        return k;
    } else if constexpr (W == 8) {
        return static_cast<uint32_t>((k * fold) >> 32);
    } else {
        const uint64_t x = k.lo ^ (k.hi * fold);
        return static_cast<uint32_t>((x * fold) >> 32);
    }
}

// host/wide.hpp wide_slots. Generic: h = x * mul, s1 = high half of h *
// slots (two quarter-rate multiplies). Narrow (keys < 2^16, slots < 65536):
// h = x * mul on 24 bits, s1 = ((h >> 8) * (slots << 8)) >> 32, both full-rate
// 24-bit multiplies. s2 = s1 ^ bits 8..15 of h (slots a multiple of 256).
// Direct (keys < 2^16, slots = 65536): s1 = s2 = x.
enum : uint32_t { kHashGeneric = 0, kHashNarrow = 1, kHashDirect = 2 };
__device__ __forceinline__ void wslots(uint32_t x, uint32_t mul, uint32_t slots, uint32_t mode, uint32_t& s1,
                                       uint32_t& s2) {
    uint32_t h;
    if (mode == kHashNarrow) {
        h = __umul24(x, mul);
        s1 = static_cast<uint32_t>((static_cast<uint64_t>(h >> 8) * ((slots << 8) & 0xFFFFFFu)) >> 32);
    } else if (mode == kHashDirect) {
        s1 = s2 = x;
        return;
    } else {
        h = x * mul;
        s1 = __umulhi(h, slots);
    }
    s2 = s1 ^ ((h >> 8) & 255u);
}

template <uint32_t W, typename V>
struct Tab {
    const Slot<KeyT<W>, V>* s;
    uint32_t slots, mul1, mode;
    uint64_t fold;
};

// the values of N letters (0 = no code), two reads per letter as above.
// Selects as masks: a select between two loaded values is otherwise turned
// into a load from a selected address (flat, through scratch).
template <typename V>
__device__ __forceinline__ V keep_if(bool c, V v) {
    return v & (V(0) - V(c));
}
template <uint32_t W, typename V, int B>
__device__ __forceinline__ void lookup_group(const Tab<W, V>& t, const KeyT<W>* key, V* val) {
    using S = Slot<KeyT<W>, V>;
    uint32_t s1[B], s2[B];
#pragma unroll
    for (int k = 0; k < B; ++k) wslots(hkey<W>(key[k], t.fold), t.mul1, t.slots, t.mode, s1[k], s2[k]);
    S e1[B];
#pragma unroll
    for (int k = 0; k < B; ++k) e1[k] = t.s[s1[k]];
    // an empty slot's key is no letter of the table (host/wide.hpp), so a
    // key match alone means the slot holds the letter
    bool m1[B];
    uint32_t a2[B];
#pragma unroll
    for (int k = 0; k < B; ++k) {
        m1[k] = key_eq(e1[k].key, key[k]);
        a2[k] = m1[k] ? 0u : s2[k];
    }
    S e2[B];
#pragma unroll
    for (int k = 0; k < B; ++k) e2[k] = t.s[a2[k]];
#pragma unroll
    for (int k = 0; k < B; ++k) val[k] = m1[k] ? e1[k].val : keep_if(key_eq(e2[k].key, key[k]), e2[k].val);
}
// in groups of <= 8 letters (4 with long values and small keys): the
// slots of a group are in flight together
template <uint32_t W, typename V, int N>
__device__ __forceinline__ void lookup_n(const Tab<W, V>& t, const KeyT<W> (&key)[N], V (&val)[N]) {
    constexpr int B0 = sizeof(V) == 8 && W <= 2 ? 4 : 8;
    constexpr int B = N < B0 ? N : B0;
#pragma unroll
    for (int g = 0; g < N; g += B) lookup_group<W, V, B>(t, key + g, val + g);
}

// bytes of letters per lane per round, and the round
// lane bytes per round (16 or 32) of pass 1 and pass 2 by letter width, and
// the rounds of loads in flight ahead of the encoder (tuning knobs)
#ifndef WIDE_LB_BITS2
#define WIDE_LB_BITS2 32
#endif
#ifndef WIDE_LB_BITS4
#define WIDE_LB_BITS4 32
#endif
#ifndef WIDE_LB_PACK2
#define WIDE_LB_PACK2 32
#endif
#ifndef WIDE_LB_PACK4
#define WIDE_LB_PACK4 32
#endif
template <uint32_t W, bool PACK>
constexpr uint32_t lane_bytes() {
    if constexpr (W == 1) return 16u;
    if constexpr (W == 2) return PACK ? WIDE_LB_PACK2 : WIDE_LB_BITS2;
    if constexpr (W == 4) return PACK ? WIDE_LB_PACK4 : WIDE_LB_BITS4;
    return 32u;
}

// letter k of the lane's bytes
template <uint32_t W, int NW>
__device__ __forceinline__ KeyT<W> letter_of(const uint32_t (&w)[NW], int k) {
    if constexpr (W == 1) {
        return (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    } else if constexpr (W == 2) {
        return (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
    } else if constexpr (W == 4) {
        return w[k];
    } else if constexpr (W == 8) {
        return w[2 * k] | (static_cast<uint64_t>(w[2 * k + 1]) << 32);
    } else {
        return U128{w[4 * k] | (static_cast<uint64_t>(w[4 * k + 1]) << 32),
                    w[4 * k + 2] | (static_cast<uint64_t>(w[4 * k + 3]) << 32)};
    }
}

template <uint32_t W>
__device__ __forceinline__ KeyT<W> letter_at(const uint8_t* __restrict__ in, uint64_t i) {
    if constexpr (W == 1) return in[i];
    else if constexpr (W == 2) return reinterpret_cast<const uint16_t*>(in)[i];
    else if constexpr (W == 4) return reinterpret_cast<const uint32_t*>(in)[i];
    else if constexpr (W == 8) return reinterpret_cast<const uint64_t*>(in)[i];
    else return U128{reinterpret_cast<const uint64_t*>(in)[2 * i], reinterpret_cast<const uint64_t*>(in)[2 * i + 1]};
}

template <typename V>
__device__ __forceinline__ uint32_t len_of(V v) {
    return static_cast<uint32_t>(v) & (sizeof(V) == 8 ? 63u : 31u);
}

__host__ __device__ constexpr uint32_t table_lds_bytes(uint32_t slots, uint32_t slot_bytes) {
    return (slots * slot_bytes + 15u) & ~15u;
}

// the table: copied into LDS (the host pads it to 16 bytes), or read in place
template <uint32_t W, typename V, bool LDS>
__device__ __forceinline__ Tab<W, V> stage_table(const WideArgs& a, uint8_t* lds) {
    using S = Slot<KeyT<W>, V>;
    // the hash form: compile-time for wide keys and for tables in LDS (those
    // of 16-bit keys are always narrow), else the table's
    const uint32_t mode = W > 2 ? kHashGeneric : (LDS ? kHashNarrow : a.hash_mode);
    Tab<W, V> t{nullptr, a.slots, a.mul1, mode, a.fold};
    if constexpr (LDS) {
        const uint32_t q = table_lds_bytes(a.slots, a.slot_bytes) / 16;
        for (uint32_t i = threadIdx.x; i < q; i += blockDim.x)
            reinterpret_cast<uint4*>(lds)[i] = static_cast<const uint4*>(a.table)[i];
        t.s = reinterpret_cast<const S*>(lds);
    } else {
        t.s = static_cast<const S*>(a.table);
    }
    return t;
}

// ---------------------------------------------------------------------------
// letter j of a 16-byte group of decoded letters
template <typename T>
__device__ __forceinline__ void put_letter(uint32_t (&w)[4], uint32_t j, T v) {
    if constexpr (sizeof(T) >= 4) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(&v);
#pragma unroll
        for (uint32_t k = 0; k < sizeof(T) / 4; ++k) w[j * (sizeof(T) / 4) + k] = p[k];
    } else {
        constexpr uint32_t per = 4 / sizeof(T);
        w[j / per] |= static_cast<uint32_t>(v) << (8 * sizeof(T) * (j % per));
    }
}
template <typename T>
__device__ __forceinline__ T get_letter(const uint32_t (&w)[4], uint32_t j) {
    if constexpr (sizeof(T) >= 4) {
        T v;
        uint32_t* p = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
        for (uint32_t k = 0; k < sizeof(T) / 4; ++k) p[k] = w[j * (sizeof(T) / 4) + k];
        return v;
    } else {
        constexpr uint32_t per = 4 / sizeof(T);
        return static_cast<T>(w[j / per] >> (8 * sizeof(T) * (j % per)));
    }
}

}  // namespace huff::dev
