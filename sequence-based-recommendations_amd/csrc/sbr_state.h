// The head every state blob starts with (include/sbr_rnn.h "Training state": sbr_state_*, sbr_cluster_state_*, sbr_dataset_state_*),
// and the two checks every load makes before it reads on.  Host code only.
#pragma once
#include "sbr_common.h"
#include <cstring>

#define SBR_STATE_MAGIC 0x3154415453524253ull      // "SBRSTAT1", little endian
#define SBR_STATE_VERSION 1u
enum { SBR_STATE_ENGINE = 1, SBR_STATE_CLUSTER = 2, SBR_STATE_DATASET = 3 };

struct SbrStateHead {
    uint64_t magic;
    uint32_t version;
    uint32_t kind;          // SBR_STATE_*
    uint64_t bytes;         // of the whole blob, this head included
};

static inline SbrStateHead sbr_state_head(uint32_t kind, size_t bytes) { return {SBR_STATE_MAGIC, SBR_STATE_VERSION, kind, (uint64_t)bytes}; }

// size (at least a head, and what the head says), magic, version, kind -- in that order; the message names the first mismatch
static inline int sbr_state_check_head(const void* blob, size_t bytes, uint32_t kind, const char* who) {
    CHECK_ARG(blob, "%s: null blob", who);
    CHECK_ARG(bytes >= sizeof(SbrStateHead), "%s: a blob of %zu bytes is shorter than its head (%zu)", who, bytes, sizeof(SbrStateHead));
    SbrStateHead hd;
    memcpy(&hd, blob, sizeof(hd));
    CHECK_ARG(hd.magic == SBR_STATE_MAGIC, "%s: wrong magic %016llx (not a state blob)", who, (unsigned long long)hd.magic);
    CHECK_ARG(hd.version == SBR_STATE_VERSION, "%s: format version %u, this library reads %u", who, hd.version, SBR_STATE_VERSION);
    CHECK_ARG(hd.kind == kind, "%s: the blob is of kind %u, expected %u (1 engine, 2 cluster head, 3 dataset)", who, hd.kind, kind);
    CHECK_ARG(hd.bytes == (uint64_t)bytes, "%s: the blob says %llu bytes, %zu were handed in (truncated?)", who, (unsigned long long)hd.bytes, bytes);
    return SBR_OK;
}
