// One view of a KV cache for the kernels of kvcache.hip, passed by value.  The three caches of halva_amd/decode.py are one thing seen
// through it:
//   plain (KVCache)    own rows only: k, v bf16 [rows, H, L, 128], lens int32 [rows]; every prefix field null / 0, anc null;
//   fork  (ForkCache)  the rows are members; member m reads parent row p = prefix_of[m] of pk, pv bf16 [.., H, Lpre, 128] up to
//                      prefix_lens[p] in front of its own rows, and own row t sits at position prefix_lens[p] + t.  prefix_of int32 [rows]
//                      is non-decreasing, prefix_lens int32 [P].  An entry that only appends brings no pk / pv / Lpre;
//   beam  (BeamCache)  a fork whose own row t of member m is held by the slot of member anc[m][t] (anc int32 [rows, L]).
// Every length lives on the device.  Slots at or beyond lens[m], and parent slots at or beyond prefix_lens[p], are never read.
#pragma once
#include "common.h"

struct CacheView {
    u32x4* k;                     // own K, V in 16-byte pieces
    u32x4* v;
    int32_t* lens;                // filled own slots per row
    int rows, H, L;
    const u32x4* pk;              // prefix rows, read only
    const u32x4* pv;
    const int32_t* prefix_lens;
    const int32_t* prefix_of;
    int P, Lpre;
    const int32_t* anc;

    // The prefix length of row m and, in p, the prefix row behind it - the one place that asks which cache this is.  Without a prefix: 0
    // (p = 0).  With one: p = -1 when prefix_of[m] names no row of [0, P); otherwise prefix_lens[p] as recorded (a negative one is the
    // caller's to refuse or to read as empty), cut to the Lpre slots of the prefix rows where the view holds them.
    __device__ __forceinline__ int prefix_len(int m, int& p) const {
        p = 0;
        if (!prefix_of) return 0;
        p = prefix_of[m];
        if (p < 0 || p >= P) {
            p = -1;
            return 0;
        }
        const int len = prefix_lens[p];
        return pk ? min(len, Lpre) : len;
    }
};
