#include "HipTextMatcher.h"

#include "pgrc_mem.h"

namespace PgTools {

    uint64_t HipTextMatcher::callsServed = 0;

    HipTextMatcher::HipTextMatcher(const char *srcText, const size_t srcLength, const uint32_t targetMatchLength,
                                   uint32_t minMatchLength) {
        int e = pgrc_mem_create(targetMatchLength, minMatchLength, -1, &ctx);
        if (e) {
            fprintf(stderr, "HipTextMatcher: %s (error %d)\n", pgrc_mem_last_error(nullptr), e);
            exit(EXIT_FAILURE);      // the reference's error convention (CopMEMMatcher.cpp:77-80)
        }
        e = pgrc_mem_set_src_ascii(ctx, srcText, srcLength);
        if (e) {
            fprintf(stderr, "HipTextMatcher: %s (error %d)\n", pgrc_mem_last_error(ctx), e);
            exit(EXIT_FAILURE);
        }
    }

    HipTextMatcher::~HipTextMatcher() {
        pgrc_mem_destroy(ctx);
    }

    void HipTextMatcher::matchTexts(vector<TextMatch> &resMatches, const string &destText, bool destIsSrc,
                                    bool revComplMatching, uint32_t minMatchLength) {
        resMatches.clear();
        pgrc_text_match *m = nullptr;
        uint64_t n = 0;
        const int e = pgrc_mem_match_texts(ctx, destText.data(), destText.length(), destIsSrc ? 1 : 0,
                                           revComplMatching ? 1 : 0, minMatchLength, &m, &n);
        if (e) {
            fprintf(stderr, "HipTextMatcher: %s (error %d)\n", pgrc_mem_last_error(ctx), e);
            exit(EXIT_FAILURE);      // e.g. "Minimal matching length cannot be smaller than K" (CopMEMMatcher.cpp:606-609)
        }
        resMatches.reserve(n);
        for (uint64_t i = 0; i < n; i++)
            resMatches.emplace_back(m[i].pos_src, m[i].length, m[i].pos_dest);
        pgrc_mem_free_matches(m);
        callsServed++;
    }

    uint64_t HipTextMatcher::markAndRemoveExactMatches(const vector<TextMatch> &matches, string &destPg, string &resPgMapOff,
                                                       string &resPgMapLen, uint32_t minMatchLength) {
        static_assert(sizeof(pgrc_text_match) == 3 * sizeof(uint64_t), "pgrc_text_match is three 64-bit words");
        vector<pgrc_text_match> in(matches.size());
        for (size_t i = 0; i < matches.size(); i++) {
            in[i].pos_src = matches[i].posSrcText;
            in[i].length = matches[i].length;
            in[i].pos_dest = matches[i].posDestText;
        }
        pgrc_mem_mapping mp;
        const int e = pgrc_mem_mark_and_remove(ctx, in.data(), in.size(), minMatchLength, (char *) destPg.data(),
                                               destPg.length(), &mp);
        if (e) {
            fprintf(stderr, "HipTextMatcher: %s (error %d)\n", pgrc_mem_last_error(ctx), e);
            exit(EXIT_FAILURE);
        }
        destPg.resize(mp.mapped_len);
        resPgMapOff.assign((const char *) mp.map_off, mp.map_off_bytes);
        resPgMapLen.assign((const char *) mp.map_len, mp.map_len_bytes);
        const uint64_t marks = mp.marks;
        pgrc_mem_free_mapping(&mp);
        return marks;
    }
}
