// The host-side rules of a paged int8 KV cache (include/asq_hip_paged.h), stated once for every entry that takes pools of pages behind a block table: the paged append
// (asq_rope_q8.hip) and the paged attention forms (asq_attn_decode.hip).  An entry fills the four numbers it was given and calls dims() where it checks its own
// dimensions (before the empty problem and the NULL rule) and shape() among its shape rules (after them); both report through asq_set_error under the entry's name.
#pragma once
#include "asq_common.h"

struct AsqPaged {
    int64_t num_pages, page_size, page_pitch, table_pitch;   // as the entry received them; page_pitch 0: dense
    int64_t page = 0;                                        // bytes a page holds: page_size * Hkv * D, set by dims()

    int64_t pitch() const { return page_pitch == 0 ? page : page_pitch; }   // bytes between pages

    // the ranges and the page-bytes overflow (Hkv and D: already within the entry's own ranges)
    int dims(const char *what, int64_t Hkv, int64_t D)
    {
        const int64_t lim = 1ll << 31;
        ASQ_REQUIRE(num_pages >= 0 && num_pages < lim && page_size >= 0 && page_size < lim && table_pitch >= 0 && table_pitch < lim, ASQ_ERR_DIM,
                    "%s: bad dims num_pages=%lld page_size=%lld table_pitch=%lld", what, (long long)num_pages, (long long)page_size, (long long)table_pitch);
        ASQ_REQUIRE(!__builtin_mul_overflow(page_size * Hkv, D, &page) && page <= (1ll << 60), ASQ_ERR_DIM, "%s: dims overflow", what);
        return ASQ_OK;
    }

    // the page size, the page pitch, a table wide enough for max_len rows per sequence, no rows without a pool
    int shape(const char *what, int64_t max_len) const
    {
        ASQ_REQUIRE(page_size > 0 && page_size % 16 == 0, ASQ_ERR_DIM, "%s: page_size must be a positive multiple of 16, got %lld", what, (long long)page_size);
        ASQ_REQUIRE(pitch() >= page && pitch() % 16 == 0 && pitch() <= (1ll << 60) / (num_pages > 0 ? num_pages : 1), ASQ_ERR_DIM,
                    "%s: page_pitch must be 0 (dense) or >= page_size * Hkv * D and a multiple of 16", what);
        ASQ_REQUIRE(max_len <= table_pitch * page_size, ASQ_ERR_DIM, "%s: max_len %lld needs more than the %lld table entries of %lld rows a sequence has", what,
                    (long long)max_len, (long long)table_pitch, (long long)page_size);
        ASQ_REQUIRE(max_len == 0 || num_pages > 0, ASQ_ERR_DIM, "%s: max_len %lld with a pool of no pages", what, (long long)max_len);
        return ASQ_OK;
    }
};
