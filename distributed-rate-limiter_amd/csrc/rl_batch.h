// rl_batch.h -- the plain argument structs of a batch that kernels of more
// than one translation unit take and the engine's host state holds: nothing
// here pulls in a kernel.
#pragma once

#include <stdint.h>

namespace rl {

struct ReqArgs {
    const uint64_t* key;
    const int64_t* ts;
    const int64_t* n;
    const uint32_t* cfg;
    const int64_t* sms;   // nullable: server clock = floor(ts / 1e6) (also in sorted order)
    uint8_t* dec;
    int64_t* rem;
    int64_t* retry;
    int64_t* reset;
    double* tok;          // nullable
    const uint8_t* fresh = nullptr;   // sorted order, nullable: the request inserted its key (REC_FRESH)
};

// Committed runs of the chain, indexed by the run's first sorted position
// (k_tb_expand's input; len is reset to 0 once the run is expanded)
struct TbRuns {
    uint16_t* len;       // requests in the run starting here (0: none), <= CH_TILE
    int16_t* E;          // decade / binade exponent (XDEC: the floor + XRUN)
    int64_t* D0;         // exact stored state before the run
    int64_t* D1;         // exact stored state after it, as the chain resolved it
    uint32_t* xlist;     // start positions of the runs of multi-decade windows (k_tb_expand_x)
    uint32_t* xcnt;      // their count (a zeroed control word of the batch set)
};

// one segment: the requests of one state-table slot, [j0, j0 + len) sorted
struct SegRec {
    uint32_t j0;
    uint32_t len;
};

// the segment work lists k_segments builds (rl_group.h) and the replay
// kernels drain (rl_replay.h)
struct SegLists {
    SegRec* list[4];
    uint32_t* count;      // 4 counters
    uint32_t* claim;      // per huge segment: claimed by a replay block (zeroed per batch)
};

}  // namespace rl
