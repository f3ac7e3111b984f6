"""ctypes binding of libpgrc_match.so (include/pgrc_match.h).

The shared library is the product: HIP kernels + C ABI.  This module only loads
it and declares the prototypes.  There is no Python / CPU fallback: if the
library is missing, import fails loudly with the build hint.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PGRC_MATCH_LIB: another build of the same library (A/B runs of compile-time variants, tools/variants.sh)
LIB_PATH = os.environ.get("PGRC_MATCH_LIB") or os.path.join(_HERE, "libpgrc_match.so")

NOT_MATCHED_POS = 0xFFFFFFFFFFFFFFFF  # DefaultReadsMatcher::NOT_MATCHED_POSITION (ReadsMatchers.cpp:69)
NOT_MATCHED_CNT = 255                 # NOT_MATCHED_COUNT (ReadsMatchers.h:17)

ERR_NAMES = {0: "OK", 1: "E_PARAM", 2: "E_SEED_SHORT", 3: "E_NO_DEVICE", 4: "E_ALLOC",
             5: "E_SYMBOL", 6: "E_STATE", 7: "E_MODE", 8: "E_DEVICE"}


class PgrcMatchError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"pgrc_match error {code} ({ERR_NAMES.get(code, '?')}): {msg}")
        self.code = code


class MatchParams(C.Structure):
    _fields_ = [("read_len", C.c_uint32), ("seed_len", C.c_uint32), ("max_mismatches", C.c_uint8),
                ("min_mismatches", C.c_uint8), ("mode", C.c_char), ("device", C.c_int32)]


class CopmemParams(C.Structure):
    _fields_ = [("K", C.c_int32), ("k1", C.c_int32), ("k2", C.c_int32), ("hash_size", C.c_uint32)]


class Counters(C.Structure):
    _fields_ = [("searched", C.c_uint64 * 2), ("candidates", C.c_uint64 * 2), ("probes", C.c_uint64 * 2),
                ("entry_fetches", C.c_uint64 * 2), ("verifies", C.c_uint64 * 2), ("index_entries", C.c_uint64 * 2), ("ms_index", C.c_float * 2), ("ms_match", C.c_float * 2),
                ("ms_other", C.c_float), ("ms_total", C.c_float), ("ms_allgather", C.c_float),
                ("screened", C.c_uint32), ("ms_screen", C.c_float), ("redo_reads", C.c_uint64), ("dual", C.c_uint64 * 5),
                ("schedule_downgraded", C.c_uint32), ("dual_seed_probes", C.c_uint64), ("dual_skip_reads", C.c_uint64),
                ("dual_rewinds", C.c_uint64)]


class SynthPg(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("pg_len", C.c_uint64), ("grid", C.c_uint32), ("plant_len", C.c_uint32),
                ("pool_div", C.c_uint32), ("tandem_every", C.c_uint32)]


class SynthReads(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("n", C.c_uint64), ("read_len", C.c_uint32), ("paired", C.c_uint32),
                ("n_with_n", C.c_uint64)]


class ExportStreams(C.Structure):   # pgrc_export_streams
    _fields_ = [("n_entries", C.c_uint64), ("n_mismatches", C.c_uint64), ("off_width", C.c_uint32), ("off", C.POINTER(C.c_uint8)),
                ("org_idx", C.POINTER(C.c_uint32)), ("rev_comp", C.POINTER(C.c_uint8)), ("mis_cnt", C.POINTER(C.c_uint8)),
                ("mis_sym", C.POINTER(C.c_uint8)), ("mis_rev_off", C.POINTER(C.c_uint8)), ("last_pos", C.c_uint64)]


class ListArchiveStreams(C.Structure):   # pgrc_list_archive_streams (include/pgrc_decode.h)
    _fields_ = [("struct_size", C.c_uint32), ("props_len", C.c_uint32), ("n_entries", C.c_uint64), ("n_mismatches", C.c_uint64),
                ("n_nonzero", C.c_uint64), ("zero_flags", C.c_void_p), ("nonzero_cnt", C.c_void_p), ("mis_sym", C.c_void_p),
                ("bases_order", C.c_char * 5), ("n_dests", C.c_uint32), ("props", C.c_void_p), ("dest", C.c_void_p * 255),
                ("dest_len", C.c_uint64 * 255), ("block", C.c_void_p)]


class ListArchiveTiming(C.Structure):    # pgrc_list_archive_timing
    _fields_ = [("struct_size", C.c_uint32), ("encode", C.c_int32), ("ms_upload", C.c_float), ("ms_flags_device", C.c_float),
                ("ms_symbols_device", C.c_float), ("ms_split_device", C.c_float), ("ms_download", C.c_float), ("ms_call", C.c_float),
                ("bytes_up", C.c_uint64), ("bytes_down", C.c_uint64), ("n_nonzero", C.c_uint64), ("limit", C.c_uint64)]


class PairOrderDecodeTiming(C.Structure):    # pgrc_pairorder_decode_timing
    _fields_ = [("struct_size", C.c_uint32), ("form", C.c_int32), ("ms_upload", C.c_float), ("ms_chain_device", C.c_float),
                ("ms_landing_device", C.c_float), ("ms_tail_device", C.c_float), ("ms_check_device", C.c_float),
                ("ms_download", C.c_float), ("ms_call", C.c_float), ("bytes_up", C.c_uint64), ("bytes_down", C.c_uint64),
                ("n_near", C.c_uint64), ("n_delta", C.c_uint64), ("n_full", C.c_uint64), ("landing_words", C.c_uint64),
                ("landing_rounds", C.c_uint64)]


class ExportPgOrderArgs(C.Structure):   # pgrc_export_pg_order_args
    _fields_ = [("order", C.c_void_p), ("n_matched", C.c_uint64), ("read_org_idx", C.c_void_p), ("list_off", C.c_void_p),
                ("list_org_idx", C.c_void_p), ("list_rev_comp", C.c_void_p), ("list_count", C.c_uint64),
                ("rev_compl_pair_file", C.c_int32), ("byte_per_read_length", C.c_int32), ("order_on_device", C.c_int32)]


class ExportOriginalOrderArgs(C.Structure):   # pgrc_export_original_order_args
    _fields_ = [("read_org_idx", C.c_void_p), ("reads_total_count", C.c_uint64), ("pair_file_mode", C.c_int32),
                ("rev_compl_pair_file", C.c_int32), ("byte_per_read_length", C.c_int32)]


class TextMatch(C.Structure):     # pgrc_text_match (include/pgrc_mem.h) = TextMatch, matching/TextMatchers.h:10-16
    _fields_ = [("pos_src", C.c_uint64), ("length", C.c_uint64), ("pos_dest", C.c_uint64)]


class DivideParams(C.Structure):
    _fields_ = [("read_len", C.c_uint32), ("error_limit", C.c_double), ("simplified_suffix_mode", C.c_int32),
                ("separate_n_reads_set", C.c_int32), ("n_reads_lq", C.c_int32), ("device", C.c_int32)]


class DividedReads(C.Structure):
    _fields_ = [("n_hq", C.c_uint64), ("n_lq", C.c_uint64), ("n_n", C.c_uint64),
                ("hq_symbols", C.c_uint32), ("lq_symbols", C.c_uint32), ("n_symbols", C.c_uint32),
                ("hq_row_bytes", C.c_uint32), ("lq_row_bytes", C.c_uint32), ("n_row_bytes", C.c_uint32),
                ("hq_rows", C.c_void_p), ("lq_rows", C.c_void_p), ("n_rows", C.c_void_p),
                ("lq_index", C.c_void_p), ("n_index", C.c_void_p)]


class MemCounters(C.Structure):
    _fields_ = [("probes", C.c_uint64), ("events", C.c_uint64), ("stale_lookups", C.c_uint64), ("ms_index", C.c_float),
                ("ms_probe", C.c_float), ("ms_sort", C.c_float), ("ms_extend", C.c_float), ("ms_host", C.c_float),
                ("ms_replay", C.c_float), ("replay_rounds", C.c_uint32), ("event_blocks", C.c_uint32)]


class MemMapping(C.Structure):   # pgrc_mem_mapping (include/pgrc_mem.h)
    _fields_ = [("mapped_len", C.c_uint64), ("marks", C.c_uint64), ("unique_matches", C.c_uint64), ("matched_symbols", C.c_uint64),
                ("map_off", C.POINTER(C.c_uint8)), ("map_off_bytes", C.c_uint64), ("map_len", C.POINTER(C.c_uint8)),
                ("map_len_bytes", C.c_uint64)]


class VarLenPart(C.Structure):   # pgrc_varlen_part (include/pgrc_varlen.h)
    _fields_ = [("ptr", C.c_void_p), ("len", C.c_uint64), ("on_device", C.c_int32)]


class VarLenTimes(C.Structure):  # pgrc_varlen_times
    _fields_ = [("ms_upload", C.c_float), ("ms_maps", C.c_float), ("ms_scan", C.c_float), ("ms_emit", C.c_float),
                ("ms_download", C.c_float), ("ms_call", C.c_float), ("symbols", C.c_uint64), ("coded_bytes", C.c_uint64),
                ("was_decode", C.c_int32)]


class AsmInput(C.Structure):    # pgrc_asm_input (include/pgrc_assemble.h)
    _fields_ = [("struct_size", C.c_uint32), ("read_len", C.c_uint32), ("symbols", C.c_uint32), ("overlap_width", C.c_uint32),
                ("n_reads", C.c_uint64), ("packed_rows", C.c_void_p), ("next_read", C.c_void_p), ("overlap", C.c_void_p),
                ("index_mapping", C.c_void_p)]


class AsmResult(C.Structure):   # pgrc_asm_result
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("pg_len", C.c_uint64), ("n_reads", C.c_uint64),
                ("cycles", C.c_uint64), ("overlap_lost", C.c_uint64), ("components", C.c_uint64), ("singles", C.c_uint64),
                ("org_idx", C.POINTER(C.c_uint32)), ("off", C.POINTER(C.c_uint16))]


class AsmTiming(C.Structure):   # pgrc_asm_timing
    _fields_ = [("struct_size", C.c_uint32), ("passes_cycles", C.c_uint32), ("passes_rank", C.c_uint32), ("ms_upload", C.c_float),
                ("ms_checks_device", C.c_float), ("ms_cycles_device", C.c_float), ("ms_rank_device", C.c_float),
                ("ms_lists_device", C.c_float), ("ms_text_device", C.c_float), ("ms_download", C.c_float), ("ms_call", C.c_float),
                ("bytes_up", C.c_uint64), ("bytes_down", C.c_uint64)]


class OvlInput(C.Structure):    # pgrc_ovl_input (include/pgrc_overlap.h)
    _fields_ = [("struct_size", C.c_uint32), ("read_len", C.c_uint32), ("symbols", C.c_uint32), ("overlap_width", C.c_uint32),
                ("n_reads", C.c_uint64), ("stop_coef", C.c_double), ("packed_rows", C.c_void_p), ("sorted_order", C.c_void_p)]


class OvlResult(C.Structure):   # pgrc_ovl_result
    _fields_ = [("struct_size", C.c_uint32), ("sweeps", C.c_uint32), ("n_reads", C.c_uint64), ("n_left", C.c_uint64),
                ("duplicates", C.c_uint64), ("links", C.c_uint64), ("next_read", C.POINTER(C.c_uint32)), ("overlap", C.c_void_p),
                ("reads_left_after", C.POINTER(C.c_uint64))]


class OvlTiming(C.Structure):   # pgrc_ovl_timing
    _fields_ = [("struct_size", C.c_uint32), ("passes", C.c_uint32), ("ms_upload", C.c_float), ("ms_order_device", C.c_float),
                ("ms_start_device", C.c_float), ("ms_merge_device", C.c_float), ("ms_pair_device", C.c_float),
                ("ms_compact_device", C.c_float), ("ms_download", C.c_float), ("ms_call", C.c_float), ("bytes_up", C.c_uint64),
                ("bytes_down", C.c_uint64)]


class OvlRuleInfo(C.Structure):  # pgrc_ovl_rule_info
    _fields_ = [("struct_size", C.c_uint32), ("rule", C.c_uint32), ("blocks", C.c_uint32), ("tail_sweeps", C.c_uint32),
                ("follower_compares", C.c_uint64), ("past_end_compares", C.c_uint64)]


OVL_RULES = {"serial": 0, "parallel": 1}     # PGRC_OVL_RULE_*


class RsetsParams(C.Structure):  # pgrc_rsets_params (include/pgrc_readsets.h)
    _fields_ = [("struct_size", C.c_uint32), ("read_len", C.c_uint32), ("separate_n_reads_set", C.c_int32), ("n_reads_lq", C.c_int32),
                ("device", C.c_int32)]


class RsetsInfo(C.Structure):    # pgrc_rsets_info
    _fields_ = [("struct_size", C.c_uint32), ("finished", C.c_uint32), ("reads_total_count", C.c_uint64), ("count", C.c_uint64 * 3),
                ("symbols", C.c_uint32 * 3), ("row_bytes", C.c_uint32 * 3), ("disposed", C.c_uint32 * 3), ("reserved", C.c_uint32)]


class RsetsTiming(C.Structure):  # pgrc_rsets_timing
    _fields_ = [("struct_size", C.c_uint32), ("edit", C.c_uint32), ("ms_checks_device", C.c_float), ("ms_desc_device", C.c_float),
                ("ms_rows_device", C.c_float), ("ms_call", C.c_float), ("rows_moved", C.c_uint64), ("bytes_moved", C.c_uint64)]


RSETS_WHICH = {"hq": 0, "lq": 1, "n": 2}     # PGRC_RSETS_*


class RlistInfo(C.Structure):    # pgrc_rlist_info (include/pgrc_readslist.h)
    _fields_ = [("struct_size", C.c_uint32), ("off_width", C.c_uint32), ("n_entries", C.c_uint64), ("n_mismatches", C.c_uint64),
                ("last_pos", C.c_uint64), ("has_rev_comp", C.c_uint32), ("has_mismatches", C.c_uint32)]


class RlistTiming(C.Structure):  # pgrc_rlist_timing
    _fields_ = [("struct_size", C.c_uint32), ("call", C.c_uint32), ("ms_fetch_device", C.c_float), ("ms_build_device", C.c_float),
                ("ms_pack_device", C.c_float), ("ms_call", C.c_float), ("bytes_up", C.c_uint64), ("bytes_down", C.c_uint64),
                ("bytes_device_copy", C.c_uint64)]


class RlistExportArgs(C.Structure):  # pgrc_rlist_export_args
    _fields_ = [("struct_size", C.c_uint32), ("order_on_device", C.c_int32), ("order", C.c_void_p), ("n_matched", C.c_uint64),
                ("read_org_idx", C.c_void_p), ("sets", C.c_void_p), ("rev_compl_pair_file", C.c_int32), ("byte_per_read_length", C.c_int32)]


class RlistArchive(C.Structure):     # pgrc_rlist_archive
    _fields_ = [("struct_size", C.c_uint32), ("off_width", C.c_uint32), ("n_entries", C.c_uint64), ("off", C.c_void_p),
                ("rev_comp", C.c_void_p), ("org_idx", C.c_void_p), ("block_bytes", C.c_uint64), ("block", C.c_void_p),
                ("archive", ListArchiveStreams)]


class RlistPairPosArgs(C.Structure):     # pgrc_rlist_pairpos_args
    _fields_ = [("struct_size", C.c_uint32), ("pos_width", C.c_uint32), ("n_total", C.c_uint64), ("hq", C.c_void_p), ("lq", C.c_void_p),
                ("n", C.c_void_p), ("hq_len", C.c_uint64), ("lq_len", C.c_uint64), ("matcher", C.c_void_p), ("read_org_idx", C.c_void_p),
                ("sets", C.c_void_p)]


class RlistExportOrgArgs(C.Structure):  # pgrc_rlist_export_org_args (include/pgrc_readslist_ord.h)
    _fields_ = [("struct_size", C.c_uint32), ("pair_file_mode", C.c_int32), ("read_org_idx", C.c_void_p), ("sets", C.c_void_p),
                ("reads_total_count", C.c_uint64), ("rev_compl_pair_file", C.c_int32), ("byte_per_read_length", C.c_int32)]


class RlistPositionsOut(C.Structure):   # pgrc_rlist_positions_out
    _fields_ = [("struct_size", C.c_uint32), ("pos_width", C.c_uint32), ("n_total", C.c_uint64), ("positions", C.c_void_p),
                ("block_bytes", C.c_uint64), ("block", C.c_void_p)]


RLIST_CALLS = {1: "set_host", 2: "from_assembly", 3: "export_pg_order", 4: "download", 5: "archive_encode", 6: "pair_order",
               7: "pair_positions", 8: "export_original_order", 9: "positions"}     # PGRC_RLIST_*

# every symbol include/pgrc_match.h and include/pgrc_mem.h declare: (name, restype, argtypes)
_P = C.c_void_p
_PROTOS = [
    ("pgrc_match_version", C.c_char_p, []),
    ("pgrc_match_derive_params", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_char, C.POINTER(MatchParams)]),
    ("pgrc_match_create", C.c_int, [C.POINTER(MatchParams), C.POINTER(_P)]),
    ("pgrc_match_create_multi", C.c_int, [C.POINTER(MatchParams), C.c_int32, C.POINTER(C.c_int32), C.POINTER(_P)]),
    ("pgrc_match_device_count", C.c_int, [C.POINTER(C.c_int32)]),
    ("pgrc_match_shard_count", C.c_int32, [_P]),
    ("pgrc_match_shard_info", C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("pgrc_match_destroy", None, [_P]),
    ("pgrc_match_last_error", C.c_char_p, [_P]),
    ("pgrc_match_set_stream", C.c_int, [_P, _P]),
    ("pgrc_match_set_pg_ascii", C.c_int, [_P, _P, C.c_uint64]),
    ("pgrc_match_set_pg_packed_device", C.c_int, [_P, _P, C.c_uint64]),
    ("pgrc_match_pack_pg_slice", C.c_int, [_P, _P, C.c_uint64, _P]),
    ("pgrc_match_set_reads_ascii", C.c_int, [_P, _P, C.c_uint64]),
    ("pgrc_match_begin_reads", C.c_int, [_P, C.c_uint64]),
    ("pgrc_match_append_reads_ascii", C.c_int, [_P, _P, C.c_uint64]),
    ("pgrc_match_end_reads", C.c_int, [_P]),
    ("pgrc_match_append_reads_packed", C.c_int, [_P, _P, C.c_uint64, C.c_int32]),
    ("pgrc_match_set_reads_packed", C.c_int, [_P, _P, C.c_uint64]),
    ("pgrc_match_set_reads_device", C.c_int, [_P, _P, C.c_uint64, C.c_uint64]),
    ("pgrc_match_words_per_read", C.c_uint32, [C.c_uint32]),
    ("pgrc_match_init_results", C.c_int, [_P]),
    ("pgrc_match_set_results", C.c_int, [_P, _P, _P, _P]),
    ("pgrc_match_run", C.c_int, [_P, C.c_int]),
    ("pgrc_match_run_pass", C.c_int, [_P, C.c_int]),
    ("pgrc_match_get_results", C.c_int, [_P, _P, _P, _P, _P, C.POINTER(C.c_uint64)]),
    ("pgrc_match_get_results_device", C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    ("pgrc_match_extract_mismatches", C.c_int, [_P, _P, _P, _P, _P]),
    ("pgrc_match_get_redo_flags", C.c_int, [_P, _P]),
    ("pgrc_match_trim_device_memory", C.c_uint64, []),
    ("pgrc_match_prepare_index", C.c_int, [_P, C.c_int32]),
    ("pgrc_match_stream_begin", C.c_int, [_P, _P, _P, _P]),
    ("pgrc_match_stream_end", C.c_int, [_P, _P, C.POINTER(C.c_uint64)]),
    ("pgrc_match_export_pg_order", C.c_int, [_P, C.POINTER(ExportPgOrderArgs), C.POINTER(ExportStreams)]),
    ("pgrc_match_export_entries", C.c_int, [_P, _P, _P, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(ExportStreams)]),
    ("pgrc_match_export_original_order", C.c_int, [_P, C.POINTER(ExportOriginalOrderArgs), C.POINTER(ExportStreams)]),
    ("pgrc_match_free_export", None, [C.POINTER(ExportStreams)]),
    ("pgrc_match_copmem_params", C.c_int, [C.c_uint32, C.c_uint64, C.POINTER(CopmemParams)]),
    ("pgrc_match_export_index", C.c_int, [_P, C.c_int, _P, _P, C.POINTER(C.c_uint64)]),
    ("pgrc_match_export_pg", C.c_int, [_P, C.c_int, _P]),
    ("pgrc_match_reload_options", C.c_int, [_P]),
    ("pgrc_match_set_profiling", C.c_int, [_P, C.c_int]),
    ("pgrc_match_get_counters", C.c_int, [_P, C.POINTER(Counters)]),
    ("pgrc_match_get_counters_sized", C.c_int, [_P, _P, C.c_size_t]),
    ("pgrc_synth_pg_host", None, [C.POINTER(SynthPg), _P]),
    ("pgrc_synth_reads_host", None, [C.POINTER(SynthPg), _P, C.POINTER(SynthReads), C.c_uint64, C.c_uint64, _P]),
    ("pgrc_synth_pg_device", C.c_int, [C.POINTER(SynthPg), _P, _P]),
    ("pgrc_synth_reads_device", C.c_int, [C.POINTER(SynthPg), _P, C.POINTER(SynthReads), C.c_uint64, C.c_uint64,
                                          _P, C.c_uint64, _P]),
    # include/pgrc_mem.h
    ("pgrc_mem_create", C.c_int, [C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(_P)]),
    ("pgrc_mem_destroy", None, [_P]),
    ("pgrc_mem_last_error", C.c_char_p, [_P]),
    ("pgrc_mem_set_src_ascii", C.c_int, [_P, _P, C.c_uint64]),
    ("pgrc_mem_match_texts", C.c_int, [_P, _P, C.c_uint64, C.c_int, C.c_int, C.c_uint32, C.POINTER(C.POINTER(TextMatch)),
                                       C.POINTER(C.c_uint64)]),
    ("pgrc_mem_free_matches", None, [C.POINTER(TextMatch)]),
    ("pgrc_mem_set_src_device", C.c_int, [_P, _P, C.c_uint64]),
    ("pgrc_mem_match_texts_device", C.c_int, [_P, _P, C.c_uint64, C.c_int, C.c_int, C.c_uint32, C.POINTER(C.POINTER(TextMatch)),
                                              C.POINTER(C.c_uint64)]),
    ("pgrc_mem_get_counters", C.c_int, [_P, C.POINTER(MemCounters)]),
    ("pgrc_mem_mark_and_remove", C.c_int, [_P, C.POINTER(TextMatch), C.c_uint64, C.c_uint32, _P, C.c_uint64, C.POINTER(MemMapping)]),
    ("pgrc_mem_free_mapping", None, [C.POINTER(MemMapping)]),
    ("pgrc_mem_mapping_timing", C.c_int, [_P, C.POINTER(C.c_float * 5)]),
    ("pgrc_mem_mark_and_remove_resident", C.c_int, [_P, C.POINTER(TextMatch), C.c_uint64, C.c_uint32, C.c_int32, C.POINTER(MemMapping)]),
    ("pgrc_mem_encode_mapped", C.c_int, [_P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64 * 3)]),
    # include/pgrc_reads.h
    ("pgrc_divider_create", C.c_int, [C.POINTER(DivideParams), C.POINTER(_P)]),
    ("pgrc_divider_destroy", None, [_P]),
    ("pgrc_divider_last_error", C.c_char_p, [_P]),
    ("pgrc_divider_run", C.c_int, [_P, _P, _P, C.c_uint64, C.POINTER(DividedReads)]),
    ("pgrc_divider_run_fastq", C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(DividedReads)]),
    ("pgrc_divider_run_text", C.c_int, [_P, C.c_int32, _P, C.c_uint64, _P, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(DividedReads)]),
    ("pgrc_divider_last_ms", C.c_int, [_P, C.POINTER(C.c_float * 3)]),
    ("pgrc_divider_last_was_terminal", C.c_int, [_P]),
]

# include/pgrc_assemble.h (kept apart from _PROTOS, which mirrors pgrc_match.h / pgrc_mem.h / pgrc_reads.h, as
# decode.py keeps include/pgrc_decode.h apart)
ASM_PROTOS = [
    ("pgrc_asm_create", C.c_int, [C.c_int32, C.POINTER(_P)]),
    ("pgrc_asm_destroy", None, [_P]),
    ("pgrc_asm_last_error", C.c_char_p, [_P]),
    ("pgrc_asm_run", C.c_int, [_P, C.POINTER(AsmInput), C.POINTER(AsmResult)]),
    ("pgrc_asm_free_result", None, [C.POINTER(AsmResult)]),
    ("pgrc_asm_get_text", C.c_int, [_P, C.c_uint64, C.c_uint64, _P]),
    ("pgrc_asm_text_device", C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_uint64)]),
    ("pgrc_asm_packed_device", C.c_int, [_P, C.POINTER(_P)]),
    ("pgrc_asm_get_timing", C.c_int, [_P, C.POINTER(AsmTiming)]),
]

# include/pgrc_overlap.h
OVL_PROTOS = [
    ("pgrc_ovl_create", C.c_int, [C.c_int32, C.POINTER(_P)]),
    ("pgrc_ovl_destroy", None, [_P]),
    ("pgrc_ovl_last_error", C.c_char_p, [_P]),
    ("pgrc_ovl_run", C.c_int, [_P, C.POINTER(OvlInput), C.POINTER(OvlResult)]),
    ("pgrc_ovl_free_result", None, [C.POINTER(OvlResult)]),
    ("pgrc_ovl_both_sides", C.c_int, [_P, _P]),
    ("pgrc_ovl_assemble", C.c_int, [_P, _P, _P, C.POINTER(AsmResult)]),
    ("pgrc_ovl_get_timing", C.c_int, [_P, C.POINTER(OvlTiming)]),
    ("pgrc_ovl_get_sweep_ms", C.c_int, [_P, C.POINTER(C.c_float), C.c_uint32]),
]

# include/pgrc_overlap.h, the rule of the sweeps (pgrc_ovl_set_rule and pgrc_ovl_get_rule_info there)
OVL_RULE_PROTOS = [
    ("pgrc_ovlrule_set", C.c_int, [_P, C.c_uint32]),
    ("pgrc_ovlrule_get_info", C.c_int, [_P, C.POINTER(OvlRuleInfo)]),
]

# include/pgrc_varlen.h
VARLEN_PROTOS = [
    ("pgrc_varlen_create", C.c_int, [_P, C.c_uint64, C.c_int32, C.POINTER(_P)]),
    ("pgrc_varlen_destroy", None, [_P]),
    ("pgrc_varlen_last_error", C.c_char_p, [_P]),
    ("pgrc_varlen_bound", C.c_uint64, [C.c_uint64]),
    ("pgrc_varlen_encode", C.c_int, [_P, C.POINTER(VarLenPart), C.c_uint32, _P, C.c_uint64, C.c_int32, C.POINTER(C.c_uint64)]),
    ("pgrc_varlen_decode", C.c_int, [_P, _P, C.c_uint64, C.c_int32, C.c_uint64, _P, C.c_int32]),
    ("pgrc_varlen_timing", C.c_int, [_P, C.POINTER(VarLenTimes)]),
]

# include/pgrc_readsets.h
RSETS_PROTOS = [
    ("pgrc_rsets_create", C.c_int, [C.POINTER(RsetsParams), C.POINTER(_P)]),
    ("pgrc_rsets_destroy", None, [_P]),
    ("pgrc_rsets_last_error", C.c_char_p, [_P]),
    ("pgrc_rsets_append", C.c_int, [_P, C.POINTER(DividedReads), C.c_uint64]),
    ("pgrc_rsets_append_divider", C.c_int, [_P, _P]),
    ("pgrc_rsets_finish", C.c_int, [_P]),
    ("pgrc_rsets_get_info", C.c_int, [_P, C.POINTER(RsetsInfo)]),
    ("pgrc_rsets_get_rows", C.c_int, [_P, C.c_int32, C.c_uint64, C.c_uint64, _P]),
    ("pgrc_rsets_get_mapping", C.c_int, [_P, C.c_int32, _P]),
    ("pgrc_rsets_dispose", C.c_int, [_P, C.c_int32]),
    ("pgrc_rsets_move_lq", C.c_int, [_P, _P, C.c_int32]),
    ("pgrc_rsets_move_by_overlap", C.c_int, [_P, _P]),
    ("pgrc_rsets_remove", C.c_int, [_P, _P, C.c_int32]),
    ("pgrc_rsets_remove_matched", C.c_int, [_P, _P]),
    ("pgrc_rsets_overlap", C.c_int, [_P, C.c_int32, _P, C.c_double, C.c_uint32, _P, C.POINTER(OvlResult)]),
    ("pgrc_rsets_to_matcher", C.c_int, [_P, _P]),
    ("pgrc_rsets_get_timing", C.c_int, [_P, C.POINTER(RsetsTiming)]),
]

# include/pgrc_readslist.h (the pair streams' structs live in decode.py, which mirrors include/pgrc_decode.h: plain pointers here)
RLIST_PROTOS = [
    ("pgrc_rlist_create", C.c_int, [C.c_int32, C.POINTER(_P)]),
    ("pgrc_rlist_destroy", None, [_P]),
    ("pgrc_rlist_last_error", C.c_char_p, [_P]),
    ("pgrc_rlist_get_info", C.c_int, [_P, C.POINTER(RlistInfo)]),
    ("pgrc_rlist_get_timing", C.c_int, [_P, C.POINTER(RlistTiming)]),
    ("pgrc_rlist_set_host", C.c_int, [_P, C.POINTER(ExportStreams)]),
    ("pgrc_rlist_from_assembly", C.c_int, [_P, _P, _P, C.c_int32]),
    ("pgrc_rlist_from_overlap", C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(AsmResult)]),
    ("pgrc_rlist_export_pg_order", C.c_int, [_P, _P, C.POINTER(RlistExportArgs)]),
    ("pgrc_rlist_download", C.c_int, [_P, C.POINTER(ExportStreams)]),
    ("pgrc_rlist_archive_encode", C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(RlistArchive)]),
    ("pgrc_rlist_archive_free", None, [C.POINTER(RlistArchive)]),
    ("pgrc_rlist_pair_order", C.c_int, [C.POINTER(_P), C.c_int32, _P]),
    ("pgrc_rlist_pair_positions", C.c_int, [C.POINTER(RlistPairPosArgs), _P]),
]

# include/pgrc_readslist_ord.h: exported by libpgrc_rlist_ord.so (the product's objects and rlistord.hip), never by libpgrc_match.so
RLIST_ORD_PROTOS = [
    ("pgrc_rlist_export_original_order", C.c_int, [_P, _P, C.POINTER(RlistExportOrgArgs)]),
    ("pgrc_rlist_archive_encode_ord", C.c_int, [_P, C.c_int32, C.POINTER(RlistArchive)]),
    ("pgrc_rlist_positions", C.c_int, [C.POINTER(RlistPairPosArgs), C.POINTER(RlistPositionsOut)]),
    ("pgrc_rlist_positions_free", None, [C.POINTER(RlistPositionsOut)]),
]
RLIST_ORD_EXPORTED_SYMBOLS = [p[0] for p in RLIST_ORD_PROTOS]
RLIST_ORD_LIB_PATH = os.environ.get("PGRC_RLIST_ORD_LIB") or os.path.join(_HERE, "libpgrc_rlist_ord.so")


class VerifyResult(C.Structure):    # pgrc_verify_result
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_int32), ("ok", C.c_int32), ("salts_used", C.c_uint32),
                ("n_source", C.c_uint64 * 2), ("n_decoded", C.c_uint64 * 2), ("mismatched_rows", C.c_uint64),
                ("first_mismatch_file", C.c_uint32), ("first_mismatch_row", C.c_uint64), ("source_unmatched", C.c_uint64),
                ("decoded_unmatched", C.c_uint64), ("undecided", C.c_uint64), ("first_source_unmatched", C.c_uint64),
                ("first_decoded_unmatched", C.c_uint64)]


class VerifyTiming(C.Structure):    # pgrc_verify_timing
    _fields_ = [("struct_size", C.c_uint32), ("salts_used", C.c_uint32), ("ms_upload", C.c_float), ("ms_fastq", C.c_float),
                ("ms_fastq_parse_device", C.c_float), ("ms_fastq_pack_device", C.c_float), ("ms_rows_device", C.c_float),
                ("ms_compare_device", C.c_float), ("ms_hash_device", C.c_float), ("ms_sort_device", C.c_float),
                ("ms_scan_device", C.c_float), ("ms_confirm_device", C.c_float), ("ms_finish", C.c_float),
                ("ms_total", C.c_float), ("bytes_up", C.c_uint64), ("bytes_resident", C.c_uint64)]


# include/pgrc_verify.h: exported by libpgrc_verify.so (the product's objects and verify.hip), never by libpgrc_match.so
_U64P = C.POINTER(C.c_uint64)
VERIFY_PROTOS = [
    ("pgrc_verify_begin", C.c_int, [_P, C.c_int32, C.POINTER(_P)]),
    ("pgrc_verify_add_rows", C.c_int, [_P, C.c_uint32, _P, C.c_uint64]),
    ("pgrc_verify_add_fastq", C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_int32, _U64P, _U64P, _U64P]),
    ("pgrc_verify_finish", C.c_int, [_P, C.POINTER(VerifyResult)]),
    ("pgrc_verify_get_timing", C.c_int, [_P, C.POINTER(VerifyTiming)]),
    ("pgrc_verify_last_error", C.c_char_p, [_P]),
    ("pgrc_verify_end", None, [_P]),
]
VERIFY_EXPORTED_SYMBOLS = [p[0] for p in VERIFY_PROTOS]
VERIFY_LIB_PATH = os.environ.get("PGRC_VERIFY_LIB") or os.path.join(_HERE, "libpgrc_verify.so")


def bind_verify(cdll: C.CDLL) -> C.CDLL:
    """the prototypes of include/pgrc_verify.h on a library that holds them (libpgrc_verify.so; the tests' libpgrc_selftest.so)"""
    for name, res, args in VERIFY_PROTOS:
        fn = getattr(cdll, name)
        fn.restype = res
        fn.argtypes = args
    return cdll


# include/pgrc_reads_text.h: exported by libpgrc_reads_text.so (libpgrc_verify.so's objects and readstext.hip) alone
READS_FASTQ, READS_FASTA, READS_LINES = 0, 1, 2
READS_FORMATS = {"fastq": READS_FASTQ, "fasta": READS_FASTA, "lines": READS_LINES}
READS_TEXT_PROTOS = [
    ("pgrc_reads_text_format", C.c_int, [C.c_int]),
    ("pgrc_verify_add_text", C.c_int, [_P, C.c_int32, _P, C.c_uint64, _P, C.c_uint64, C.c_int32, _U64P, _U64P, _U64P]),
]
READS_TEXT_EXPORTED_SYMBOLS = [p[0] for p in READS_TEXT_PROTOS]
READS_TEXT_LIB_PATH = os.environ.get("PGRC_READS_TEXT_LIB") or os.path.join(_HERE, "libpgrc_reads_text.so")


class HufTimes(C.Structure):     # pgrc_huf_times (include/pgrc_huf.h)
    _fields_ = [("ms_upload", C.c_float), ("ms_tables", C.c_float), ("ms_emit", C.c_float), ("ms_compact", C.c_float),
                ("ms_download", C.c_float), ("ms_call", C.c_float), ("bytes", C.c_uint64), ("coded_bytes", C.c_uint64),
                ("chunks", C.c_uint32), ("huf_chunks", C.c_uint32), ("rle_chunks", C.c_uint32), ("raw_chunks", C.c_uint32),
                ("was_decode", C.c_int32)]


# include/pgrc_huf.h: exported by libpgrc_huf.so (the product's objects and huf.hip) alone
HUF_ORDER_MAX, HUF_TABLE_LOG_MIN, HUF_TABLE_LOG_MAX = 17, 8, 11
HUF_PROTOS = [
    ("pgrc_huf_create", C.c_int, [C.c_int32, C.POINTER(_P)]),
    ("pgrc_huf_destroy", None, [_P]),
    ("pgrc_huf_last_error", C.c_char_p, [_P]),
    ("pgrc_huf_bound", C.c_uint64, [C.c_uint64, C.c_uint32]),
    ("pgrc_huf_encode", C.c_int, [_P, _P, C.c_uint64, C.c_int32, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.c_int32, C.POINTER(C.c_uint64)]),
    ("pgrc_huf_decode", C.c_int, [_P, _P, C.c_uint64, C.c_int32, C.c_uint64, _P, C.c_int32]),
    ("pgrc_huf_timing", C.c_int, [_P, C.POINTER(HufTimes)]),
]
HUF_EXPORTED_SYMBOLS = [p[0] for p in HUF_PROTOS]
HUF_LIB_PATH = os.environ.get("PGRC_HUF_LIB") or os.path.join(_HERE, "libpgrc_huf.so")


def reads_format(fmt) -> int:
    """"fastq" / "fasta" / "lines" or a PGRC_READS_* number -> the number"""
    return READS_FORMATS[fmt.lower()] if isinstance(fmt, str) else int(fmt)


EXPORTED_SYMBOLS = [p[0] for p in _PROTOS]
RLIST_EXPORTED_SYMBOLS = [p[0] for p in RLIST_PROTOS]
RSETS_EXPORTED_SYMBOLS = [p[0] for p in RSETS_PROTOS]
VARLEN_EXPORTED_SYMBOLS = [p[0] for p in VARLEN_PROTOS]
ASM_EXPORTED_SYMBOLS = [p[0] for p in ASM_PROTOS]
OVL_EXPORTED_SYMBOLS = [p[0] for p in OVL_PROTOS]
OVL_RULE_EXPORTED_SYMBOLS = [p[0] for p in OVL_RULE_PROTOS]


def _preload_torch_hip_runtime() -> None:
    """One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64.so (SONAME
    libamdhip64.so.7, the same as /opt/rocm's).  If our library pulled in the system copy first and
    torch its bundled copy later, two runtimes would fight over the device (the second one reports no
    devices).  Loading torch's copy first -- without importing torch -- makes both resolve to it.
    Processes without torch (e.g. the C++ reference with the adapter) use the system runtime."""
    if os.environ.get("PGRC_USE_SYSTEM_HIP") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec and spec.origin:
            p = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
            if os.path.exists(p):
                C.CDLL(p, mode=C.RTLD_GLOBAL)
    except Exception:  # torch absent or unloadable: fall through to the system runtime
        pass


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension is the product and there is no fallback. "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C pgrc_amd/csrc`.")
    _preload_torch_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    for name, res, args in _PROTOS + ASM_PROTOS + OVL_PROTOS + OVL_RULE_PROTOS + VARLEN_PROTOS + RSETS_PROTOS + RLIST_PROTOS:
        fn = getattr(lib, name)  # AttributeError here = header / library out of sync: fail loudly
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()
if not os.path.exists(VERIFY_LIB_PATH):
    raise ImportError(f"{VERIFY_LIB_PATH} is missing: `make -C pgrc_amd/csrc` builds it beside libpgrc_match.so")
vlib = bind_verify(C.CDLL(VERIFY_LIB_PATH))
if not os.path.exists(READS_TEXT_LIB_PATH):
    raise ImportError(f"{READS_TEXT_LIB_PATH} is missing: `make -C pgrc_amd/csrc` builds it beside libpgrc_match.so")
tlib = C.CDLL(READS_TEXT_LIB_PATH)
for _name, _res, _args in READS_TEXT_PROTOS:
    _fn = getattr(tlib, _name)
    _fn.restype = _res
    _fn.argtypes = _args
if not os.path.exists(RLIST_ORD_LIB_PATH):
    raise ImportError(f"{RLIST_ORD_LIB_PATH} is missing: `make -C pgrc_amd/csrc` builds it beside libpgrc_match.so")
olib = C.CDLL(RLIST_ORD_LIB_PATH)
for _name, _res, _args in RLIST_ORD_PROTOS:
    _fn = getattr(olib, _name)
    _fn.restype = _res
    _fn.argtypes = _args
if not os.path.exists(HUF_LIB_PATH):
    raise ImportError(f"{HUF_LIB_PATH} is missing: `make -C pgrc_amd/csrc` builds it beside libpgrc_match.so")
hlib = C.CDLL(HUF_LIB_PATH)
for _name, _res, _args in HUF_PROTOS:
    _fn = getattr(hlib, _name)
    _fn.restype = _res
    _fn.argtypes = _args
