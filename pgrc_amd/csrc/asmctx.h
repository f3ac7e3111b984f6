// asmctx.h -- what pgovl.hip uses of pgasm.hip: the assembly run on an overlap graph that is already on the device
#pragma once

#include "pgrc_assemble.h"

// pgrc_asm_run with in->packed_rows, in->next_read and in->overlap in DEVICE memory of the context's device (complete when the
// call is made); in->index_mapping stays a host pointer.  Everything else as pgrc_asm_run.
int pgasm_run_device(pgrc_asm_ctx *a, const pgrc_asm_input *in, pgrc_asm_result *out);
// the same without the page-locked block and its copy: out->org_idx and out->off stay NULL, the reads list stays on the device
// (rlistctx.h: pgasm_last_list)
int pgasm_run_device_resident(pgrc_asm_ctx *a, const pgrc_asm_input *in, pgrc_asm_result *out);
int pgasm_device(const pgrc_asm_ctx *a);    // the HIP device of the context
