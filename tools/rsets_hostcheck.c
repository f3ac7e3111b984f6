/* Stand-alone check of the host side of include/pgrc_readsets.h for a sanitizer build: the parameter errors every entry point
 * answers before it touches a device.  Build the library's sources with the host sanitizers and link this program against it:
 *   make -C pgrc_amd/csrc OBJDIR=/tmp/rsets_asan/obj OUT=/tmp/rsets_asan/libpgrc_match.so SELFTEST=/tmp/rsets_asan/libpgrc_selftest.so \
 *        EXTRA="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
 *   hipcc -fsanitize=address,undefined -Iinclude tools/rsets_hostcheck.c -o /tmp/rsets_asan/hostcheck -L/tmp/rsets_asan -lpgrc_match -Wl,-rpath,/tmp/rsets_asan
 *   /tmp/rsets_asan/hostcheck
 * Meant for a machine WITHOUT a HIP device (a sanitizer-instrumented host build does not belong on a GPU machine): it covers what
 * every entry point answers in front of pgrc_rsets_create's device query -- NULL objects and pointers, struct sizes, the read
 * length -- and that create itself ends with PGRC_E_NO_DEVICE.  An object cannot exist without a device, so the state errors and
 * the parameter errors that need an object are the GPU tests' (tests/test_gpu_rsets.py), not this program's. */
#include <stdio.h>
#include <string.h>

#include "pgrc_readsets.h"

static int failures = 0;
#define EXPECT(call, want)                                                         \
    do {                                                                           \
        const int got__ = (call);                                                  \
        if (got__ != (want)) { printf("FAIL %s: %d, expected %d\n", #call, got__, (int)(want)); failures++; } \
    } while (0)

int main(void) {
    pgrc_rsets *s = NULL;
    pgrc_rsets_params p;
    pgrc_rsets_info info;
    pgrc_rsets_timing tm;
    pgrc_divided_reads batch;
    pgrc_ovl_result res;
    uint8_t flags[4] = {0, 1, 0, 1};
    uint32_t map[8];
    int e;
    memset(&batch, 0, sizeof batch);
    memset(&info, 0, sizeof info);
    memset(&tm, 0, sizeof tm);
    EXPECT(pgrc_rsets_create(NULL, NULL), PGRC_E_PARAM);
    EXPECT(pgrc_rsets_create(NULL, &s), PGRC_E_PARAM);
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p - 1;
    p.read_len = 100;
    p.device = -1;
    EXPECT(pgrc_rsets_create(&p, &s), PGRC_E_PARAM);
    p.struct_size = sizeof p;
    p.read_len = 0;
    EXPECT(pgrc_rsets_create(&p, &s), PGRC_E_PARAM);
    p.read_len = 256;
    EXPECT(pgrc_rsets_create(&p, &s), PGRC_E_PARAM);
    if (!pgrc_rsets_last_error(NULL) || !strstr(pgrc_rsets_last_error(NULL), "read length")) { printf("FAIL last_error(NULL)\n"); failures++; }
    pgrc_rsets_destroy(NULL);
    EXPECT(pgrc_rsets_append(NULL, &batch, 0), PGRC_E_PARAM);
    EXPECT(pgrc_rsets_append_divider(NULL, NULL), PGRC_E_PARAM);
    EXPECT(pgrc_rsets_finish(NULL), PGRC_E_PARAM);
    EXPECT(pgrc_rsets_get_info(NULL, &info), PGRC_E_PARAM);
    EXPECT(pgrc_rsets_get_rows(NULL, PGRC_RSETS_HQ, 0, 1, flags), PGRC_E_PARAM);
    EXPECT(pgrc_rsets_get_mapping(NULL, PGRC_RSETS_LQ, map), PGRC_E_PARAM);
    EXPECT(pgrc_rsets_dispose(NULL, PGRC_RSETS_N), PGRC_E_PARAM);
    EXPECT(pgrc_rsets_move_lq(NULL, flags, 0), PGRC_E_PARAM);
    EXPECT(pgrc_rsets_move_by_overlap(NULL, NULL), PGRC_E_PARAM);
    EXPECT(pgrc_rsets_remove(NULL, flags, 0), PGRC_E_PARAM);
    EXPECT(pgrc_rsets_remove_matched(NULL, NULL), PGRC_E_PARAM);
    EXPECT(pgrc_rsets_overlap(NULL, PGRC_RSETS_HQ, NULL, 1.0, 1, NULL, &res), PGRC_E_PARAM);
    EXPECT(pgrc_rsets_to_matcher(NULL, NULL), PGRC_E_PARAM);
    EXPECT(pgrc_rsets_get_timing(NULL, &tm), PGRC_E_PARAM);
    p.read_len = 21;
    p.separate_n_reads_set = 1;
    e = pgrc_rsets_create(&p, &s);
    if (e == PGRC_OK) {         /* a device is present: nothing more to do here */
        pgrc_rsets_destroy(s);
        printf("a HIP device is present: %d failures in the checks in front of it\n", failures);
        return failures != 0;
    }
    EXPECT(e, PGRC_E_NO_DEVICE);
    if (s) { printf("FAIL a failed create left an object\n"); failures++; }
    printf("no HIP device (%s): %d failures\n", pgrc_rsets_last_error(NULL), failures);
    return failures != 0;
}
