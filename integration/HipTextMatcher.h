// HipTextMatcher -- the reference-side binding of libpgrc_match.so for pseudogenome-vs-pseudogenome exact matching:
// a TextMatcher (matching/TextMatchers.h:53-61) that SimplePgMatcher can hold instead of its CopMEMMatcher
// (matching/SimplePgMatcher.cpp:12-19) and that forwards matchTexts to the MI355X library through the C ABI of
// include/pgrc_mem.h.
//
// NEW code for the PgRC tree (not part of the reference), compiled against the reference's headers.
#ifndef PGTOOLS_HIPTEXTMATCHER_H
#define PGTOOLS_HIPTEXTMATCHER_H

#include "matching/TextMatchers.h"

struct pgrc_mem_ctx;

namespace PgTools {

    class HipTextMatcher : public TextMatcher {
    private:
        pgrc_mem_ctx *ctx = nullptr;

    public:
        // same arguments as CopMEMMatcher(srcText, srcLength, targetMatchLength, minMatchLength)
        // (matching/copmem/CopMEMMatcher.h:79); srcText is borrowed, like CopMEMMatcher::start1
        HipTextMatcher(const char *srcText, const size_t srcLength, const uint32_t targetMatchLength,
                       uint32_t minMatchLength = UINT32_MAX);

        ~HipTextMatcher() override;

        void matchTexts(vector<TextMatch> &resMatches, const string &destText, bool destIsSrc, bool revComplMatching,
                        uint32_t minMatchLength) override;

        // The second half of SimplePgMatcher::markAndRemoveExactMatches (matching/SimplePgMatcher.cpp:85-143) on the device, for the
        // destination of the last matchTexts call: `matches` as that call returned them (BEFORE
        // correctDestPositionDueToRevComplMatching and resolveMappingCollisionsInTheSameText: the library applies both), destPg
        // the text in its forward orientation -- only its storage is used: the mapped text is written over it and it is
        // resized, as the reference's memmove loop leaves it.  minMatchLength: UINT32_MAX = the target length.
        // -> the number of marks
        uint64_t markAndRemoveExactMatches(const vector<TextMatch> &matches, string &destPg, string &resPgMapOff,
                                           string &resPgMapLen, uint32_t minMatchLength = UINT32_MAX);

        static uint64_t callsServed;     // diagnostics / tests
    };
}

#endif //PGTOOLS_HIPTEXTMATCHER_H
