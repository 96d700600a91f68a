"""ctypes binding of libcopgpu.so (the C ABI in include/cop_gpu.h).

This is the Python face of the drop-in boundary: tests and bench.py call
the HIP pipeline only through these C entry points. There is no CPU
fallback: if libcopgpu.so is missing, importing this module raises.
"""
from __future__ import annotations

import ctypes
import errno
import os
from ctypes import (POINTER, Structure, byref, c_char_p, c_double, c_int, c_int32,
                    c_size_t, c_uint8, c_uint16, c_uint32, c_uint64, c_void_p)

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libcopgpu.so")

# ---------------------------------------------------------------------------
# constants (include/cop_gpu.h)
STAGE_PARSE, STAGE_FW, STAGE_LPM = 0x1, 0x2, 0x4
FORWARD, DROP_FW, DROP_PARSE, DROP_NOT_IPV4, DROP_NO_PORT = 0, 1, 2, 3, 4
FLAG_ROUTE_HIT, FLAG_FW_HIT = 0x1, 0x2
COUNTER_SHARDS = 256   # COP_COUNTER_SHARDS
LPM_STOP_AT_FIRST_ERROR = 0x1
CFG_FW_FORCE_DIR24, CFG_LPM_FORCE_DIR24, CFG_NO_COMPACT, CFG_RULE_COUNTERS = 0x1, 0x2, 0x4, 0x8
CFG_DEMUX_PORTS, CFG_PORT_STATS, CFG_LPM_TRIE, CFG_SEG_LISTS = 0x10, 0x20, 0x40, 0x80
CFG_LPM_BKT = 0x100
CFG_FW_BKT = 0x200
CFG_LIVE_TABLES = 0x400   # the stage tables accept update_* patches (cop_update_*)
SEG_PKTS = 256   # COP_SEG_PKTS: packets per forward-list segment (CFG_SEG_LISTS)
MAX_DEMUX_PORTS = 8
GEN_FW, GEN_ROUTES = 0, 1
UNKNOWN_PORT = 0xFFFF
HDR16_STRIDE = 16   # packed header records: frame bytes 12..15 + 24..35 per packet
HDR12_STRIDE = 12   # compact records (one-shot batches): frame bytes 12..15 + 26..33 per packet

PREFIX_DT = np.dtype([("ip", "<u4"), ("next_hop", "<u4"), ("depth", "u1"), ("_pad", "u1", (3,))])
RESULT_DT = np.dtype([("verdict", "u1"), ("flags", "u1"), ("port", "<u2"), ("route_nh", "<u4")])
COUNTER_NAMES = ["pkt_drop", "pkt_accept", "pkt_not_ipv4", "pkt_total", "parse_err", "no_port",
                 "forward", "route_hit", "rx"]


class CopError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__(f"cop error {code}: {msg}")
        self.code = code


class LpmConfig(Structure):
    _fields_ = [("max_rules", c_uint32), ("number_tbl8s", c_uint32), ("flags", c_uint32)]


class LpmReport(Structure):
    _fields_ = [("n_in", c_uint32), ("n_added", c_uint32), ("n_distinct", c_uint32),
                ("n_updated", c_uint32), ("n_failed", c_uint32), ("n_skipped", c_uint32),
                ("first_error", c_int32), ("first_error_idx", c_uint32), ("tbl8_used", c_uint32),
                ("n_intervals", c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class UpdateReport(Structure):
    _fields_ = [("full", c_uint32), ("n_changes", c_uint32), ("n_records", c_uint32),
                ("tbl24_entries", c_uint32), ("tbl8_entries", c_uint32), ("groups_taken", c_uint32),
                ("groups_released", c_uint32), ("h2d_bytes", c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class AuditReport(Structure):
    """cop_audit_report (cop_lookup_audit)."""
    _fields_ = [("n_probes", c_uint64), ("n_mismatch", c_uint64), ("generation_table", c_uint64),
                ("generation_device", c_uint64), ("stale", c_uint32), ("form", c_uint32),
                ("first_ip", c_uint32), ("first_device", c_uint32), ("first_host", c_uint32),
                ("n_bad", c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# bulk lookups (cop_lookup_bulk): the output word and the two image forms
LOOKUP_HIT, LOOKUP_DROP = 0x01000000, 0x04000000
LOOKUP_NH, LOOKUP_RULE = 0, 1
LOOKUP_STAGE_WORDS = 1 << 20   # cop_internal.h: addresses per staging chunk of lookup_bulk_host / lookup_audit

PATCH_REC_DT = np.dtype([("table", "<u4"), ("first", "<u4"), ("count", "<u4"), ("entry", "<u4")])


class Config(Structure):
    _fields_ = [("device", c_int), ("stages", c_uint32), ("n_ports", c_uint32),
                ("max_batch", c_uint32), ("max_batches", c_uint32), ("flags", c_uint32),
                ("n_streams", c_uint32), ("routing_table", POINTER(c_uint16))]


class Batch(Structure):
    _fields_ = [("pkts", c_void_p), ("offsets", c_void_p), ("n", c_uint32), ("stride", c_uint32),
                ("data_off", c_uint32), ("_pad", c_uint32), ("results", c_void_p),
                ("fwd_idx", c_void_p), ("fwd_count", c_void_p)]


class BatchRing(Structure):
    _fields_ = [("pkts", c_void_p), ("offsets", c_void_p), ("results", c_void_p), ("fwd_idx", c_void_p),
                ("fwd_count", c_void_p), ("pkts_slot_bytes", c_uint64), ("offsets_slot_words", c_uint64),
                ("results_slot", c_uint64), ("fwd_slot", c_uint64), ("n_slots", c_uint32), ("n", c_uint32),
                ("stride", c_uint32), ("data_off", c_uint32)]


TX_MAX_FRAME = 2048   # COP_TX_MAX_FRAME


class TxBurst(Structure):
    _fields_ = [("frames", c_void_p), ("off", c_void_p), ("len", c_void_p), ("status", c_void_p),
                ("cap_bytes", c_uint64), ("cap_frames", c_uint32), ("_pad", c_uint32)]


class TxDesc(Structure):
    _fields_ = [("lens", c_void_p), ("copy_bytes", c_uint32), ("slot_bytes", c_uint32),
                ("out", TxBurst * MAX_DEMUX_PORTS)]


SKETCH_MAX_ROWS = 4    # COP_SKETCH_MAX_ROWS
SKETCH_KEY_SRC, SKETCH_KEY_DST = 0, 1


class SketchConfig(Structure):
    _fields_ = [("rows", c_uint32), ("log2_cols", c_uint32), ("key", c_uint32), ("key_depth", c_uint32),
                ("seed", c_uint64)]


class PoliceDesc(Structure):
    _fields_ = [("threshold", c_uint64), ("out_idx", c_void_p), ("out_count", c_void_p), ("status", c_void_p)]


AEAD_TAG_BYTES = 16    # COP_AEAD_TAG_BYTES


class AeadKey(Structure):
    _fields_ = [("key", ctypes.c_uint8 * 32), ("salt", ctypes.c_uint8 * 4), ("_pad", c_uint32)]


class AeadBurst(Structure):
    _fields_ = [("frames", c_void_p), ("off", c_void_p), ("len", c_void_p), ("count", c_void_p), ("tags", c_void_p),
                ("ok", c_void_p), ("status", c_void_p), ("cap_bytes", c_uint64), ("seq_base", c_uint64),
                ("n_frames", c_uint32), ("slot_bytes", c_uint32), ("frame_bytes", c_uint32), ("aad_bytes", c_uint32)]


NEIGH_VALID = 0x1        # COP_NEIGH_VALID
FWD_OK, FWD_PASS, FWD_SHORT, FWD_BAD_HDR, FWD_OPTIONS, FWD_BAD_CSUM, FWD_TTL, FWD_NO_NEIGH = range(8)   # COP_FWD_*
FWD_VERIFY_CSUM = 0x1    # cop_fwd_config.flags
FWD_NO_NH = 0xFFFFFFFF   # COP_FWD_NO_NH
NEIGH_DT = np.dtype([("dst_mac", "u1", (6,)), ("src_mac", "u1", (6,)), ("port", "<u2"), ("flags", "<u2")])


class NeighEntry(Structure):
    _fields_ = [("dst_mac", ctypes.c_uint8 * 6), ("src_mac", ctypes.c_uint8 * 6), ("port", ctypes.c_uint16),
                ("flags", ctypes.c_uint16)]


class FwdConfig(Structure):
    _fields_ = [("flags", c_uint32), ("miss_nh", c_uint32)]


class FwdCheckDesc(Structure):
    _fields_ = [("lens", c_void_p), ("out_idx", c_void_p), ("out_count", c_void_p), ("exc_idx", c_void_p),
                ("exc_count", c_void_p), ("status", c_void_p)]


class FwdRwDesc(Structure):
    _fields_ = [("port", c_void_p * MAX_DEMUX_PORTS), ("status", c_void_p * MAX_DEMUX_PORTS)]


ACL_MAX_RULES = 1024     # COP_ACL_MAX_RULES
ACL_HIT, ACL_DROP, ACL_SKIP = 0x01000000, 0x04000000, 0x08000000   # COP_ACL_*
ACL_COUNTERS = 0x1       # cop_acl_create flag
ACL_RULE_DT = np.dtype([("src_ip", "<u4"), ("dst_ip", "<u4"), ("sport_lo", "<u2"), ("sport_hi", "<u2"),
                        ("dport_lo", "<u2"), ("dport_hi", "<u2"), ("src_depth", "u1"), ("dst_depth", "u1"),
                        ("proto", "u1"), ("proto_mask", "u1"), ("priority", "<i4"), ("action", "<u4")])
ACL_KEY_DT = np.dtype([("src", "<u4"), ("dst", "<u4"), ("sport", "<u2"), ("dport", "<u2"), ("proto", "u1"),
                       ("_pad", "u1", (3,))])


class AclReport(Structure):
    _fields_ = [("n_rules", c_uint32), ("n_intervals", c_uint32 * 4), ("row_words", c_uint32),
                ("first_error_idx", c_uint32), ("_pad", c_uint32), ("image_bytes", c_uint64)]


class AclDesc(Structure):
    _fields_ = [("words", c_void_p), ("out_idx", c_void_p), ("out_count", c_void_p), ("status", c_void_p)]


class TraceOpts(Structure):
    _fields_ = [("n_ports", c_uint32), ("pct_non_ipv4", c_uint32), ("pct_bad_version", c_uint32),
                ("pct_unknown_dst", c_uint32), ("pct_vport_dst", c_uint32),
                ("pct_src_in_rule", c_uint32)]


class PmdInfo(Structure):
    _fields_ = [("workers", c_uint32), ("workers_per_cu", c_uint32), ("tiles_per_batch", c_uint32),
                ("packets_per_tile", c_uint32), ("launches", c_uint32), ("state", c_uint32),
                ("posted", c_uint64), ("completed", c_uint64), ("slot_loads", c_uint32), ("kernel", c_uint32)]


class NfStats(Structure):
    _fields_ = [("rx_packets", c_uint64), ("rx_dropped", c_uint64), ("tx_packets", c_uint64),
                ("tx_dropped", c_uint64)]


class PortStats(Structure):
    _fields_ = [("rx_packets", c_uint64), ("rx_dropped", c_uint64), ("tx_packets", c_uint64),
                ("tx_dropped", c_uint64), ("nf_dropped", c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# every function declared in include/cop_gpu.h: name -> (restype, argtypes)
SIGNATURES = {
    "cop_lpm_build": (c_int, [c_void_p, c_uint32, POINTER(LpmConfig), POINTER(c_void_p), POINTER(LpmReport)]),
    "cop_lpm_free": (None, [c_void_p]),
    "cop_lpm_export_dir24": (c_int, [c_void_p, c_void_p, c_void_p, c_uint32]),
    "cop_lpm_export_intervals": (c_int, [c_void_p, c_void_p, c_void_p, c_uint32]),
    "cop_lpm_export_rules": (c_int, [c_void_p, c_void_p, c_uint32]),
    "cop_lpm_lookup_rules": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p]),
    "cop_lpm_create": (c_int, [POINTER(LpmConfig), POINTER(c_void_p)]),
    "cop_lpm_add": (c_int, [c_void_p, c_uint32, c_uint8, c_uint32]),
    "cop_lpm_delete": (c_int, [c_void_p, c_uint32, c_uint8]),
    "cop_lpm_delete_all": (c_int, [c_void_p]),
    "cop_lpm_is_rule_present": (c_int, [c_void_p, c_uint32, c_uint8, POINTER(c_uint32)]),
    "cop_lpm_generation": (c_uint64, [c_void_p]),
    "cop_lpm_export_rules_ids": (c_int, [c_void_p, c_void_p, c_void_p, c_uint32]),
    "cop_update_fw_table": (c_int, [c_void_p, c_void_p, POINTER(UpdateReport)]),
    "cop_update_route_lpm": (c_int, [c_void_p, c_void_p, POINTER(UpdateReport)]),
    "cop_update_fw_rules_file": (c_int, [c_void_p, c_void_p, c_char_p, POINTER(UpdateReport)]),
    "cop_replace_fw_table": (c_int, [c_void_p, c_void_p, POINTER(UpdateReport)]),
    "cop_replace_route_lpm": (c_int, [c_void_p, c_void_p, POINTER(UpdateReport)]),
    "cop_lpm_lookup_words": (c_int, [c_void_p, c_int, c_void_p, c_uint32, c_void_p]),
    "cop_lookup_bulk": (c_int, [c_void_p, c_uint32, c_void_p, c_uint32, c_void_p]),
    "cop_lookup_bulk_host": (c_int, [c_void_p, c_uint32, c_void_p, c_uint64, c_void_p]),
    "cop_lookup_audit": (c_int, [c_void_p, c_uint32, c_void_p, POINTER(AuditReport), c_void_p, c_uint32]),
    "cop_tx_gather": (c_int, [c_void_p, POINTER(Batch), POINTER(TxDesc), c_uint32]),
    "cop_submit_tx": (c_int, [c_void_p, POINTER(Batch), POINTER(TxDesc), c_uint32]),
    "cop_tx_gather_host": (c_int, [POINTER(Batch), POINTER(TxDesc), c_uint32, c_uint32, c_int, c_uint32]),
    "cop_sketch_create": (c_int, [c_void_p, POINTER(SketchConfig), POINTER(c_void_p)]),
    "cop_sketch_destroy": (c_int, [c_void_p, c_void_p]),
    "cop_sketch_update": (c_int, [c_void_p, c_void_p, POINTER(Batch), c_uint32, c_uint32]),
    "cop_sketch_query": (c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_void_p]),
    "cop_sketch_police": (c_int, [c_void_p, c_void_p, POINTER(Batch), POINTER(PoliceDesc), c_uint32]),
    "cop_sketch_decay": (c_int, [c_void_p, c_void_p, c_uint32]),
    "cop_sketch_read": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64]),
    "cop_sketch_device_ptr": (c_int, [c_void_p, c_void_p, POINTER(c_void_p), POINTER(c_uint64)]),
    "cop_sketch_params": (c_int, [POINTER(SketchConfig), POINTER(c_uint32), POINTER(c_uint32)]),
    "cop_sketch_update_host": (c_int, [POINTER(SketchConfig), c_void_p, POINTER(Batch), c_uint32, c_uint32, c_uint32]),
    "cop_sketch_query_host": (c_int, [POINTER(SketchConfig), c_void_p, c_void_p, c_uint32, c_void_p]),
    "cop_sketch_police_host": (c_int, [POINTER(SketchConfig), c_void_p, POINTER(Batch), POINTER(PoliceDesc), c_uint32,
                                       c_uint32, c_int, c_uint32]),
    "cop_aead_seal": (c_int, [c_void_p, POINTER(AeadKey), POINTER(AeadBurst), c_uint32]),
    "cop_aead_open": (c_int, [c_void_p, POINTER(AeadKey), POINTER(AeadBurst), c_uint32]),
    "cop_aead_seal_host": (c_int, [POINTER(AeadKey), POINTER(AeadBurst), c_uint32]),
    "cop_aead_open_host": (c_int, [POINTER(AeadKey), POINTER(AeadBurst), c_uint32]),
    "cop_chacha20_block_host": (None, [c_void_p, c_uint32, c_void_p, c_void_p]),
    "cop_poly1305_host": (None, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "cop_poly1305_bulk": (c_int, [c_void_p, POINTER(AeadBurst), c_void_p]),
    "cop_rules_load_json": (c_int, [c_char_p, POINTER(c_void_p), POINTER(c_uint32)]),
    "cop_rules_free": (None, [c_void_p]),
    "cop_rules_write_json": (c_int, [c_char_p, c_void_p, c_uint32]),
    "cop_rules_load_bin": (c_int, [c_char_p, POINTER(c_void_p), POINTER(c_uint32)]),
    "cop_rules_write_bin": (c_int, [c_char_p, c_void_p, c_uint32]),
    "cop_route_table_default": (None, [c_void_p, c_uint32]),
    "cop_config_default": (None, [POINTER(Config)]),
    "cop_create": (c_int, [POINTER(Config), POINTER(c_void_p)]),
    "cop_destroy": (None, [c_void_p]),
    "cop_last_error": (c_char_p, [c_void_p]),
    "cop_device_count": (c_int, []),
    "cop_device_pci_bus_id": (c_int, [c_int, ctypes.c_char_p, c_int]),
    "cop_set_fw_table": (c_int, [c_void_p, c_void_p]),
    "cop_set_route_lpm": (c_int, [c_void_p, c_void_p]),
    "cop_set_routing_table": (c_int, [c_void_p, c_void_p]),
    "cop_load_fw_rules_file": (c_int, [c_void_p, c_char_p, POINTER(LpmConfig), POINTER(LpmReport)]),
    "cop_submit": (c_int, [c_void_p, POINTER(Batch), c_uint32]),
    "cop_submit_ring": (c_int, [c_void_p, POINTER(BatchRing), c_uint32, c_uint32]),
    "cop_sync": (c_int, [c_void_p]),
    "cop_pmd_start": (c_int, [c_void_p, POINTER(BatchRing), POINTER(c_void_p)]),
    "cop_pmd_post": (c_int, [c_void_p, c_uint32]),
    "cop_pmd_wait": (c_int, [c_void_p, c_uint64]),
    "cop_pmd_posted": (c_uint64, [c_void_p]),
    "cop_pmd_run": (c_int, [c_void_p, c_uint64]),
    "cop_pmd_run_timed": (c_int, [c_void_p, c_uint64, POINTER(c_uint64), POINTER(c_uint64)]),
    "cop_pmd_info": (c_int, [c_void_p, POINTER(PmdInfo)]),
    "cop_pmd_stop": (c_int, [c_void_p]),
    "cop_pmd_start_rings": (c_int, [c_void_p, POINTER(BatchRing), c_uint32, c_uint32, POINTER(c_void_p)]),
    "cop_pmd_post_ring": (c_int, [c_void_p, c_uint32, c_uint32]),
    "cop_pmd_post_batch": (c_int, [c_void_p, c_uint32, c_uint32]),
    "cop_pmd_wait_ring": (c_int, [c_void_p, c_uint32, c_uint64]),
    "cop_pmd_posted_ring": (c_uint64, [c_void_p, c_uint32]),
    "cop_pmd_completed_ring": (c_uint64, [c_void_p, c_uint32]),
    "cop_poll": (c_int, [c_void_p]),
    "cop_process_host": (c_int, [c_void_p, POINTER(c_void_p), c_uint32, c_void_p, c_void_p, c_void_p]),
    "cop_process_host_stream": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_void_p]),
    "cop_set_host_threads": (c_int, [c_void_p, c_uint32]),
    "cop_pack_headers": (None, [c_void_p, c_uint32, c_void_p]),
    "cop_pack_headers12": (None, [c_void_p, c_uint32, c_void_p]),
    "cop_counters_read": (c_int, [c_void_p, c_void_p, c_int]),
    "cop_counters_device_ptr": (c_void_p, [c_void_p]),
    "cop_rule_counters_read": (c_int, [c_void_p, c_void_p, c_uint32, c_int]),
    "cop_port_stats_read": (c_int, [c_void_p, POINTER(PortStats), c_uint32, c_int]),
    "cop_counters_snapshot": (c_int, [c_void_p, c_void_p, POINTER(PortStats), c_uint32, c_int]),
    "cop_rule_counters_device_ptr": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_uint32)]),
    "cop_coll_unique_id": (c_int, [c_void_p]),
    "cop_coll_init": (c_int, [c_void_p, c_void_p, c_int, c_int]),
    "cop_coll_reduce_counters": (c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_int]),
    "cop_neigh_create": (c_int, [c_void_p, c_uint32, POINTER(c_void_p)]),
    "cop_neigh_set": (c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_void_p]),
    "cop_neigh_destroy": (c_int, [c_void_p, c_void_p]),
    "cop_neigh_device_ptr": (c_int, [c_void_p, c_void_p, POINTER(c_void_p), POINTER(c_uint32)]),
    "cop_fwd_check": (c_int, [c_void_p, c_void_p, POINTER(FwdConfig), POINTER(Batch), POINTER(FwdCheckDesc), c_uint32]),
    "cop_fwd_rewrite": (c_int, [c_void_p, c_void_p, POINTER(FwdConfig), POINTER(Batch), POINTER(TxDesc),
                                POINTER(FwdRwDesc), c_uint32]),
    "cop_fwd_check_host": (c_int, [c_void_p, c_uint32, POINTER(FwdConfig), POINTER(Batch), POINTER(FwdCheckDesc),
                                   c_uint32, c_uint32, c_int, c_uint32]),
    "cop_fwd_rewrite_host": (c_int, [c_void_p, c_uint32, POINTER(FwdConfig), POINTER(Batch), POINTER(TxDesc),
                                     POINTER(FwdRwDesc), c_uint32, c_uint32, c_int, c_uint32]),
    "cop_ipv4_csum_host": (ctypes.c_uint16, [c_void_p]),
    "cop_acl_build": (c_int, [c_void_p, c_uint32, POINTER(c_void_p), POINTER(AclReport)]),
    "cop_acl_free": (None, [c_void_p]),
    "cop_acl_match_host": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p]),
    "cop_acl_create": (c_int, [c_void_p, c_void_p, c_uint32, POINTER(c_void_p)]),
    "cop_acl_set": (c_int, [c_void_p, c_void_p, c_void_p]),
    "cop_acl_destroy": (c_int, [c_void_p, c_void_p]),
    "cop_acl_counters_read": (c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_int]),
    "cop_acl_device_ptr": (c_int, [c_void_p, c_void_p, POINTER(c_void_p), POINTER(c_uint64), POINTER(c_void_p),
                                   POINTER(c_uint32)]),
    "cop_acl_classify": (c_int, [c_void_p, c_void_p, POINTER(Batch), POINTER(AclDesc), c_uint32]),
    "cop_acl_filter": (c_int, [c_void_p, c_void_p, POINTER(Batch), POINTER(AclDesc), c_uint32]),
    "cop_acl_classify_host": (c_int, [c_void_p, POINTER(Batch), POINTER(AclDesc), c_uint32, c_uint32]),
    "cop_acl_filter_host": (c_int, [c_void_p, c_void_p, POINTER(Batch), POINTER(AclDesc), c_uint32, c_uint32, c_int,
                                    c_uint32]),
    "cop_dev_alloc": (c_int, [c_void_p, c_size_t, POINTER(c_void_p)]),
    "cop_dev_alloc_ex": (c_int, [c_void_p, c_size_t, c_uint32, POINTER(c_void_p)]),
    "cop_dev_free": (c_int, [c_void_p, c_void_p]),
    "cop_host_alloc_pinned": (c_int, [c_void_p, c_size_t, POINTER(c_void_p)]),
    "cop_host_alloc_mapped": (c_int, [c_void_p, c_size_t, POINTER(c_void_p), POINTER(c_void_p)]),
    "cop_host_free_pinned": (c_int, [c_void_p, c_void_p]),
    "cop_memcpy_h2d": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    "cop_memcpy_d2h": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    "cop_memcpy_d2d": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    "cop_memset_d": (c_int, [c_void_p, c_void_p, c_int, c_size_t]),
    "cop_timer_start": (c_int, [c_void_p]),
    "cop_timer_stop": (c_int, [c_void_p, POINTER(c_double)]),
    "cop_launch_timing": (c_int, [c_void_p, c_int]),
    "cop_launch_timing_read": (c_int, [c_void_p, POINTER(c_double), POINTER(c_uint64), c_int]),
    "cop_ring_create": (c_void_p, [c_uint32]),
    "cop_ring_free": (None, [c_void_p]),
    "cop_ring_enqueue_bulk": (c_uint32, [c_void_p, c_void_p, c_uint32, POINTER(c_uint32)]),
    "cop_ring_dequeue_burst": (c_uint32, [c_void_p, c_void_p, c_uint32, POINTER(c_uint32)]),
    "cop_ring_count": (c_uint32, [c_void_p]),
    "cop_set_mbuf_layout": (None, [c_uint32, c_uint32]),
    "cop_set_rule_file": (None, [c_char_p]),
    "coprocessor_setup": (c_int, []),
    "cop_set_dropin_stages": (c_int, [c_uint32]),
    "cop_dropin_stages": (c_uint32, []),
    "cop_coprocessor_setup_stages": (c_int, [c_uint32]),
    "cop_coprocessor_setup_fw": (c_int, []),
    "cop_coprocessor_setup_no_nf": (c_int, []),
    "coprocessor_teardown": (c_int, []),
    "process_packet": (c_int, [c_void_p]),
    "process_burst": (c_int, [c_void_p, c_uint32, c_void_p]),
    "cop_coprocessor_poll": (c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, POINTER(NfStats)]),
    "cop_coprocessor_poll_async": (c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p,
                                           POINTER(NfStats)]),
    "cop_coprocessor_flush": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(NfStats)]),
    "cop_pmd_host_create": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32, POINTER(c_void_p)]),
    "cop_coprocessor_poll_pmd": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p,
                                         POINTER(NfStats)]),
    "cop_coprocessor_flush_pmd": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, POINTER(NfStats)]),
    "cop_pmd_host_destroy": (c_int, [c_void_p]),
    "cop_host_batch_submit": (c_int, [c_void_p, c_uint32, c_void_p, c_uint32]),
    "cop_host_batch_wait": (c_int, [c_void_p, c_uint32, POINTER(c_void_p), POINTER(c_uint32)]),
    "coprocessor_ctx": (c_void_p, []),
    "cop_gen_rules": (c_int, [c_uint64, c_uint32, c_int, c_uint32, c_void_p]),
    "cop_trace_opts_default": (None, [POINTER(TraceOpts)]),
    "cop_gen_trace": (c_int, [c_uint64, c_uint32, POINTER(TraceOpts), c_void_p, c_uint32, c_void_p,
                              c_uint32, c_void_p, c_uint32]),
    "cop_gen_imix": (c_int, [c_uint64, c_uint32, POINTER(TraceOpts), c_void_p, c_uint32, c_void_p,
                             c_uint32, c_void_p, POINTER(c_uint64), c_void_p]),
}

_lib = None


def lib():
    """Load libcopgpu.so (raises ImportError when it has not been built)."""
    global _lib
    if _lib is None:
        # $COP_LIB: an alternative in-tree build of the same ABI (A/B runs)
        path = os.environ.get("COP_LIB") or LIB_PATH
        if not os.path.exists(path):
            raise ImportError(f"{path} not built (run make -C ghost-dataplane_amd)")
        L = ctypes.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("COP_LIB") and not hasattr(L, name):
                continue   # an older A/B build: calls it lacks fail when used
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(c_void_p) if a is not None else None


def _check(rc, ctx=None, what=""):
    if rc < 0:
        msg = what
        if ctx is not None and ctx.handle:
            msg += ": " + lib().cop_last_error(ctx.handle).decode(errors="replace")
        raise CopError(rc, msg)
    return rc


# ---------------------------------------------------------------------------
# host helpers

def pack_headers(ptrs: np.ndarray) -> np.ndarray:
    """cop_pack_headers over host packet addresses (u64 array): n x 16 bytes."""
    ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
    out = np.zeros(len(ptrs) * HDR16_STRIDE, np.uint8)
    lib().cop_pack_headers(ptrs.ctypes.data, len(ptrs), out.ctypes.data)
    return out


def pack_headers_np(frames: np.ndarray, n: int, stride: int = 64) -> np.ndarray:
    """The same records from a contiguous frame array, in numpy (tests)."""
    f = np.asarray(frames, np.uint8)[: n * stride].reshape(n, stride)
    return np.ascontiguousarray(np.concatenate([f[:, 12:16], f[:, 24:36]], axis=1)).reshape(-1)


def pack_headers12(ptrs: np.ndarray) -> np.ndarray:
    """cop_pack_headers12 over host packet addresses (u64 array): n x 12 bytes."""
    ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
    out = np.zeros(len(ptrs) * HDR12_STRIDE, np.uint8)
    lib().cop_pack_headers12(ptrs.ctypes.data, len(ptrs), out.ctypes.data)
    return out


def prefixes(ip, depth, next_hop) -> np.ndarray:
    ip = np.asarray(ip, dtype=np.uint64)
    a = np.zeros(len(ip), dtype=PREFIX_DT)
    a["ip"] = ip.astype(np.uint32)
    a["depth"] = np.asarray(depth, dtype=np.int64).astype(np.uint8)
    a["next_hop"] = np.asarray(next_hop, dtype=np.uint64).astype(np.uint32)
    return a


def gen_rules(seed: int, n: int, kind: int = GEN_FW, n_long_parents: int = 20) -> np.ndarray:
    out = np.zeros(n, dtype=PREFIX_DT)
    _check(lib().cop_gen_rules(seed, n, kind, n_long_parents, _ptr(out)), what="gen_rules")
    return out


def trace_opts(**kw) -> TraceOpts:
    o = TraceOpts()
    lib().cop_trace_opts_default(byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def gen_trace(seed: int, n: int, fw=None, routes=None, stride: int = 64, opts: TraceOpts | None = None,
              out: np.ndarray | None = None) -> np.ndarray:
    if out is None:
        out = np.zeros(n * stride, dtype=np.uint8)
    fw = fw if fw is not None else np.zeros(0, dtype=PREFIX_DT)
    routes = routes if routes is not None else np.zeros(0, dtype=PREFIX_DT)
    _check(lib().cop_gen_trace(seed, n, byref(opts) if opts else None, _ptr(fw), len(fw), _ptr(routes),
                               len(routes), _ptr(out), stride), what="gen_trace")
    return out


def gen_imix(seed: int, n: int, fw=None, routes=None, opts: TraceOpts | None = None):
    fw = fw if fw is not None else np.zeros(0, dtype=PREFIX_DT)
    routes = routes if routes is not None else np.zeros(0, dtype=PREFIX_DT)
    size = c_uint64(0)
    o = byref(opts) if opts else None
    _check(lib().cop_gen_imix(seed, n, o, _ptr(fw), len(fw), _ptr(routes), len(routes), None, byref(size), None))
    slab = np.zeros(size.value + 64, dtype=np.uint8)
    offs = np.zeros(n, dtype=np.uint32)
    _check(lib().cop_gen_imix(seed, n, o, _ptr(fw), len(fw), _ptr(routes), len(routes), _ptr(slab),
                              byref(size), _ptr(offs)))
    return slab, offs


def route_table_default(n_ports: int = 5) -> np.ndarray:
    rt = np.zeros(65536, dtype=np.uint16)
    lib().cop_route_table_default(_ptr(rt), n_ports)
    return rt


def rules_load_json(path: str) -> np.ndarray:
    p = c_void_p()
    n = c_uint32()
    _check(lib().cop_rules_load_json(path.encode(), byref(p), byref(n)), what=f"load {path}")
    try:
        buf = (ctypes.c_uint8 * (n.value * PREFIX_DT.itemsize)).from_address(p.value) if n.value else b""
        return np.frombuffer(bytes(buf), dtype=PREFIX_DT).copy()
    finally:
        lib().cop_rules_free(p)


def rules_write_json(path: str, rules: np.ndarray):
    rules = np.ascontiguousarray(rules, dtype=PREFIX_DT)
    _check(lib().cop_rules_write_json(path.encode(), _ptr(rules), len(rules)), what=f"write {path}")


def rules_load_bin(path: str) -> np.ndarray:
    """Binary prefix dump (cop_rules_load_bin) -> PREFIX_DT array."""
    p = c_void_p()
    n = c_uint32()
    _check(lib().cop_rules_load_bin(path.encode(), byref(p), byref(n)), what=f"load {path}")
    try:
        buf = (ctypes.c_uint8 * (n.value * PREFIX_DT.itemsize)).from_address(p.value) if n.value else b""
        return np.frombuffer(bytes(buf), dtype=PREFIX_DT).copy()
    finally:
        lib().cop_rules_free(p)


def rules_write_bin(path: str, rules: np.ndarray):
    rules = np.ascontiguousarray(rules, dtype=PREFIX_DT)
    _check(lib().cop_rules_write_bin(path.encode(), _ptr(rules), len(rules)), what=f"write {path}")


class LpmTable:
    """Host-built LPM table with DPDK rte_lpm_add semantics."""

    def __init__(self, rules: np.ndarray, max_rules=1024, number_tbl8s=24, stop_at_first_error=True):
        rules = np.ascontiguousarray(rules, dtype=PREFIX_DT)
        cfg = LpmConfig(max_rules, number_tbl8s, LPM_STOP_AT_FIRST_ERROR if stop_at_first_error else 0)
        self.handle = c_void_p()
        self.report = LpmReport()
        _check(lib().cop_lpm_build(_ptr(rules), len(rules), byref(cfg), byref(self.handle),
                                   byref(self.report)), what="cop_lpm_build")

    def __del__(self):
        if getattr(self, "handle", None) and self.handle.value:
            lib().cop_lpm_free(self.handle)
            self.handle = c_void_p()

    @classmethod
    def empty(cls, max_rules=1024, number_tbl8s=24) -> "LpmTable":
        """An empty table (cop_lpm_create) to fill with add()."""
        t = cls.__new__(cls)
        cfg = LpmConfig(max_rules, number_tbl8s, 0)
        t.handle = c_void_p()
        t.report = LpmReport()
        _check(lib().cop_lpm_create(byref(cfg), byref(t.handle)), what="cop_lpm_create")
        t._refresh()
        return t

    def _refresh(self):
        """self.report as the table is now (n_distinct, tbl8_used, n_intervals)."""
        f = lib().cop_lpm_report_get
        f.restype = None
        f.argtypes = [c_void_p, POINTER(LpmReport)]
        f(self.handle, byref(self.report))

    def add(self, ip: int, depth: int, next_hop: int) -> int:
        """rte_lpm_add: 0, or -EINVAL / -ENOSPC with the table unchanged."""
        if not 0 <= depth <= 255:
            return -22
        rc = lib().cop_lpm_add(self.handle, ip & 0xFFFFFFFF, depth, next_hop & 0xFFFFFFFF)
        self._refresh()
        return rc

    def delete(self, ip: int, depth: int) -> int:
        """rte_lpm_delete: 0, or -EINVAL (bad depth, or the rule is not held)."""
        if not 0 <= depth <= 255:
            return -22
        rc = lib().cop_lpm_delete(self.handle, ip & 0xFFFFFFFF, depth)
        self._refresh()
        return rc

    def delete_all(self) -> int:
        rc = lib().cop_lpm_delete_all(self.handle)
        self._refresh()
        return rc

    def is_rule_present(self, ip: int, depth: int):
        """(1, next hop), (0, None) or (-EINVAL, None)."""
        if not 0 <= depth <= 255:
            return -22, None
        nh = c_uint32(0)
        rc = lib().cop_lpm_is_rule_present(self.handle, ip & 0xFFFFFFFF, depth, byref(nh))
        return rc, (nh.value if rc == 1 else None)

    @property
    def generation(self) -> int:
        return int(lib().cop_lpm_generation(self.handle))

    def rules_ids(self):
        """(rules, ids): every held rule with its rule id (the index of its
        per-rule counter), in id order."""
        n = _check(lib().cop_lpm_export_rules_ids(self.handle, None, None, 0))
        out = np.zeros(n, dtype=PREFIX_DT)
        ids = np.zeros(n, dtype=np.uint32)
        _check(lib().cop_lpm_export_rules_ids(self.handle, _ptr(out), _ptr(ids), n))
        return out, ids

    # -- patches for a device DIR-24-8 image (cop_internal.h; tests, tools) --
    def live_image(self, form: int = 0, cap_groups: int | None = None) -> "LiveImage":
        """The freshly painted DIR-24-8 image of a form (0: next hop, 1: rule
        id) with room for cap_groups tbl8 groups, and its book of groups."""
        return LiveImage(self, form, cap_groups)

    def journal_set_cap(self, cap: int):
        f = lib().cop_lpm_journal_set_cap
        f.restype = c_int
        f.argtypes = [c_void_p, c_uint32]
        _check(f(self.handle, cap), what="cop_lpm_journal_set_cap")

    def rules(self) -> np.ndarray:
        n = _check(lib().cop_lpm_export_rules(self.handle, None, 0))
        out = np.zeros(n, dtype=PREFIX_DT)
        _check(lib().cop_lpm_export_rules(self.handle, _ptr(out), n))
        return out

    def lookup_rules(self, ips: np.ndarray) -> np.ndarray:
        """Matching rule id per address (-1 on a miss), host-side."""
        ips = np.ascontiguousarray(ips, dtype=np.uint32)
        out = np.zeros(len(ips), dtype=np.int32)
        _check(lib().cop_lpm_lookup_rules(self.handle, _ptr(ips), len(ips), _ptr(out)))
        return out

    def lookup_words(self, ips: np.ndarray, form: int = LOOKUP_NH) -> np.ndarray:
        """cop_lpm_lookup_words: per address the exact word cop_lookup_bulk
        returns (LOOKUP_NH: next hop | LOOKUP_HIT; LOOKUP_RULE: rule id |
        LOOKUP_HIT | LOOKUP_DROP; 0 on a miss), from the host table as it is now."""
        ips = np.ascontiguousarray(ips, dtype=np.uint32)
        out = np.zeros(len(ips), dtype=np.uint32)
        _check(lib().cop_lpm_lookup_words(self.handle, form, _ptr(ips), len(ips), _ptr(out)), what="cop_lpm_lookup_words")
        return out

    def audit_probes(self, form: int = LOOKUP_NH) -> np.ndarray:
        """cop_lookup_audit's probe set for this table (cop_internal.h; tests)."""
        f = lib().cop_lpm_audit_probes
        f.restype = c_int
        f.argtypes = [c_void_p, c_int, POINTER(c_void_p), POINTER(c_uint32)]
        p, n = c_void_p(), c_uint32(0)
        _check(f(self.handle, form, byref(p), byref(n)), what="cop_lpm_audit_probes")
        try:
            return np.frombuffer(bytes((ctypes.c_uint8 * (n.value * 4)).from_address(p.value)), dtype=np.uint32).copy()
        finally:
            ctypes.CDLL(None).free(p)

    def intervals(self):
        m = _check(lib().cop_lpm_export_intervals(self.handle, None, None, 1 << 31))
        s = np.zeros(m, dtype=np.uint32)
        v = np.zeros(m, dtype=np.uint32)
        _check(lib().cop_lpm_export_intervals(self.handle, _ptr(s), _ptr(v), m))
        return s, v

    def trie_probe(self, ips: np.ndarray, form: int = 0):
        """The multibit-trie form (lpm_trie.c) of this table's device image
        (form 0: next hop, 1: rule id), walked on the host: (trie values,
        interval-search values, nodes, leaves) for each address."""
        ips = np.ascontiguousarray(ips, dtype=np.uint32)
        out = np.zeros(len(ips), dtype=np.uint32)
        ref = np.zeros(len(ips), dtype=np.uint32)
        nn, nl = ctypes.c_uint32(), ctypes.c_uint32()
        f = lib().cop_lpm_trie_probe
        f.restype = c_int
        f.argtypes = [c_void_p, c_int, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]
        _check(f(self.handle, form, _ptr(ips), len(ips), _ptr(out), _ptr(ref), byref(nn), byref(nl)),
               what="cop_lpm_trie_probe")
        return out, ref, nn.value, nl.value

    def bkt_probe(self, ips: np.ndarray, form: int = 0, xbits: int = 1):
        """The bucketed interval form (lpm_bkt.c) of this table's device
        image (form 0: next hop, 1: rule id), looked up on the host the way
        the kernel does: (values, interval-search values, info dict)."""
        ips = np.ascontiguousarray(ips, dtype=np.uint32)
        out = np.zeros(len(ips), dtype=np.uint32)
        ref = np.zeros(len(ips), dtype=np.uint32)
        info = np.zeros(6, dtype=np.uint32)
        f = lib().cop_lpm_bkt_probe
        f.restype = c_int
        f.argtypes = [c_void_p, c_int, c_uint32, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p]
        _check(f(self.handle, form, xbits, _ptr(ips), len(ips), _ptr(out), _ptr(ref), _ptr(info)), what="cop_lpm_bkt_probe")
        return out, ref, dict(zip(("m", "ib", "lv", "widest", "lifted", "rounds"), (int(x) for x in info)))

    def dir24(self):
        t24 = np.zeros(1 << 24, dtype=np.uint32)
        cap = 256 * max(1, self.report.n_distinct)
        t8 = np.zeros(cap, dtype=np.uint32)
        n_ext = _check(lib().cop_lpm_export_dir24(self.handle, _ptr(t24), _ptr(t8), cap))
        return t24, t8[: n_ext * 256]


class LiveImage:
    """Host copy of a patched DIR-24-8 image: tbl24 / tbl8 arrays, the book
    of tbl8 groups (cop_live_img) and the table generation they hold.
    records() returns the fill records that bring the image to the table's
    current generation (and moves the book there); apply() is the host mirror
    of the patch kernel."""

    def __init__(self, table: LpmTable, form: int = 0, cap_groups: int | None = None):
        L = lib()
        self.table, self.form = table, form
        L.cop_lpm_form_n_ext.restype = c_uint32
        L.cop_lpm_form_n_ext.argtypes = [c_void_p, c_int]
        n_ext = L.cop_lpm_form_n_ext(table.handle, form)
        self.cap_groups = n_ext + 64 if cap_groups is None else cap_groups
        self.tbl24 = np.zeros(1 << 24, dtype=np.uint32)
        self.tbl8 = np.zeros(max(self.cap_groups, n_ext, 1) * 256, dtype=np.uint32)
        L.cop_lpm_form_fill_dir24.restype = None
        L.cop_lpm_form_fill_dir24.argtypes = [c_void_p, c_int, c_void_p, c_void_p]
        L.cop_lpm_form_fill_dir24(table.handle, form, _ptr(self.tbl24), _ptr(self.tbl8))
        L.cop_live_img_create.restype = c_void_p
        L.cop_live_img_create.argtypes = [c_void_p, c_int, c_uint32]
        self.handle = c_void_p(L.cop_live_img_create(table.handle, form, self.cap_groups))
        if not self.handle.value:
            raise CopError(-12, "cop_live_img_create")

    def __del__(self):
        if getattr(self, "handle", None) and self.handle.value:
            f = lib().cop_live_img_free
            f.restype = None
            f.argtypes = [c_void_p]
            f(self.handle)
            self.handle = c_void_p()

    def records(self):
        """(records, report dict), or (None, -errno): -ESTALE (-116) when the
        journal no longer reaches back, -ENOSPC (-28) when the groups ran out."""
        f = lib().cop_lpm_patch_records
        f.restype = c_int
        f.argtypes = [c_void_p, c_void_p, POINTER(c_void_p), POINTER(c_uint32), POINTER(UpdateReport)]
        p, n, rep = c_void_p(), c_uint32(0), UpdateReport()
        rc = f(self.table.handle, self.handle, byref(p), byref(n), byref(rep))
        if rc < 0:
            return None, rc
        try:
            buf = (ctypes.c_uint8 * (n.value * PATCH_REC_DT.itemsize)).from_address(p.value) if n.value else b""
            recs = np.frombuffer(bytes(buf), dtype=PATCH_REC_DT).copy()
        finally:
            ctypes.CDLL(None).free(p)
        return recs, rep.as_dict()

    def apply(self, recs: np.ndarray):
        patch_apply_host(self.tbl24, self.tbl8, recs)

    def lookup(self, ips: np.ndarray) -> np.ndarray:
        """The image's entry for each address (tbl24, then its tbl8 group)."""
        ips = np.asarray(ips, dtype=np.uint32)
        e = self.tbl24[ips >> 8]
        ext = (e & 0x03000000) == 0x03000000
        g = (e[ext] & 0x00FFFFFF).astype(np.int64)
        e = e.copy()
        e[ext] = self.tbl8[g * 256 + (ips[ext] & 0xFF)]
        return e


def patch_apply_host(tbl24: np.ndarray, tbl8: np.ndarray, recs: np.ndarray):
    """cop_patch_apply_host: fill records into host arrays (the kernel's mirror)."""
    recs = np.ascontiguousarray(recs, dtype=PATCH_REC_DT)
    f = lib().cop_patch_apply_host
    f.restype = c_int
    f.argtypes = [c_void_p, c_uint32, c_void_p, c_uint32, c_void_p, c_uint32]
    _check(f(_ptr(tbl24), len(tbl24), _ptr(tbl8), len(tbl8), _ptr(recs), len(recs)), what="cop_patch_apply_host")


PAINT_CHUNK = 4096   # cop_kernels.h COPK_PAINT_CHUNK: /24 blocks per workgroup of the paint kernel


def paint_plan(table: LpmTable, form: int = 0):
    """cop_lpm_paint_plan: (starts, entries, ext24) of a form (0: next hop,
    1: rule id), the paint kernel's inputs; len(ext24) is the form's n_ext."""
    f = lib().cop_lpm_paint_plan
    f.restype = c_int
    f.argtypes = [c_void_p, c_int, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_uint32), POINTER(c_void_p),
                  POINTER(c_uint32)]
    ps, pe, px, niv, n_ext = c_void_p(), c_void_p(), c_void_p(), c_uint32(0), c_uint32(0)
    _check(f(table.handle, form, byref(ps), byref(pe), byref(niv), byref(px), byref(n_ext)), what="cop_lpm_paint_plan")

    def take(p, n):
        try:
            return np.frombuffer(bytes((ctypes.c_uint8 * (n * 4)).from_address(p.value)), dtype=np.uint32).copy()
        finally:
            ctypes.CDLL(None).free(p)
    return take(ps, niv.value), take(pe, niv.value), take(px, n_ext.value)


def paint_host(starts: np.ndarray, entries: np.ndarray, ext24: np.ndarray, cap_groups: int, fill: int = 0):
    """cop_paint_host, the paint kernel's mirror: (tbl24, tbl8) with tbl8 of
    cap_groups * 256 entries, both pre-filled with `fill`."""
    starts = np.ascontiguousarray(starts, dtype=np.uint32)
    entries = np.ascontiguousarray(entries, dtype=np.uint32)
    ext24 = np.ascontiguousarray(ext24, dtype=np.uint32)
    assert len(starts) == len(entries)
    t24 = np.full(1 << 24, fill, dtype=np.uint32)
    t8 = np.full(max(cap_groups, 1) * 256, fill, dtype=np.uint32)
    f = lib().cop_paint_host
    f.restype = c_int
    f.argtypes = [c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p, c_void_p, c_uint32]
    _check(f(_ptr(starts), _ptr(entries), len(starts), _ptr(ext24) if len(ext24) else None, len(ext24), _ptr(t24),
             _ptr(t8), cap_groups), what="cop_paint_host")
    return t24, t8[: cap_groups * 256]


ALLOC_UNCACHED, ALLOC_FINEGRAINED = 1, 2


class DeviceBuffer:
    def __init__(self, ctx: "Context", nbytes: int, flags: int = 0):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        self.ptr = c_void_p()
        if flags:
            _check(lib().cop_dev_alloc_ex(ctx.handle, self.nbytes, flags, byref(self.ptr)), ctx, "dev_alloc_ex")
        else:
            _check(lib().cop_dev_alloc(ctx.handle, self.nbytes, byref(self.ptr)), ctx, "dev_alloc")

    @property
    def addr(self) -> int:
        return self.ptr.value

    def upload(self, a: np.ndarray, offset: int = 0):
        a = np.ascontiguousarray(a)
        assert offset + a.nbytes <= self.nbytes
        _check(lib().cop_memcpy_h2d(self.ctx.handle, c_void_p(self.addr + offset), _ptr(a), a.nbytes),
               self.ctx, "h2d")

    def download(self, dtype, count: int, offset: int = 0) -> np.ndarray:
        out = np.zeros(count, dtype=dtype)
        assert offset + out.nbytes <= self.nbytes
        if out.nbytes:
            _check(lib().cop_memcpy_d2h(self.ctx.handle, _ptr(out), c_void_p(self.addr + offset), out.nbytes),
                   self.ctx, "d2h")
        return out

    def fill(self, value: int = 0):
        _check(lib().cop_memset_d(self.ctx.handle, self.ptr, value, self.nbytes), self.ctx, "memset")

    def free(self):
        if self.ptr.value:
            lib().cop_dev_free(self.ctx.handle, self.ptr)
            self.ptr = c_void_p()

    def __del__(self):
        try:
            if self.ptr.value and self.ctx.handle:
                self.free()
        except Exception:
            pass


COLL_ID_BYTES = 128


def coll_unique_id() -> bytes:
    """RCCL unique id (rank 0 creates it; the caller distributes it)."""
    buf = (c_uint8 * COLL_ID_BYTES)()
    _check(lib().cop_coll_unique_id(buf), what="cop_coll_unique_id")
    return bytes(buf)


def device_count() -> int:
    return lib().cop_device_count()


def device_pci_bus_id(device: int) -> str:
    buf = ctypes.create_string_buffer(64)
    _check(lib().cop_device_pci_bus_id(device, buf, 64), what="cop_device_pci_bus_id")
    return buf.value.decode().lower()


class Context:
    """One GPU context (cop_ctx): device, stream, NF tables."""

    def __init__(self, device=0, stages=STAGE_PARSE | STAGE_FW, n_ports=5, max_batch=262144,
                 max_batches=32, flags=0, routing_table: np.ndarray | None = None, n_streams=None):
        cfg = Config()
        lib().cop_config_default(byref(cfg))
        cfg.device, cfg.stages, cfg.n_ports = device, stages, n_ports
        cfg.max_batch, cfg.max_batches, cfg.flags = max_batch, max_batches, flags
        if n_streams is not None:
            cfg.n_streams = n_streams
        self._rt = None
        if routing_table is not None:
            self._rt = np.ascontiguousarray(routing_table, dtype=np.uint16)
            cfg.routing_table = self._rt.ctypes.data_as(POINTER(c_uint16))
        self.handle = c_void_p()
        rc = lib().cop_create(byref(cfg), byref(self.handle))
        if rc < 0:
            raise CopError(rc, "cop_create failed (no GPU?)")
        self.cfg = cfg

    def close(self):
        if self.handle and self.handle.value:
            for m in getattr(self, "_pmds", []):
                m.stop()
            lib().cop_destroy(self.handle)
            self.handle = c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_fw_table(self, t: LpmTable):
        _check(lib().cop_set_fw_table(self.handle, t.handle), self, "set_fw_table")

    def set_route_lpm(self, t: LpmTable):
        _check(lib().cop_set_route_lpm(self.handle, t.handle), self, "set_route_lpm")

    ROUTE_FORMS = {1: "lds", 2: "dir", 3: "trie", 4: "bkt"}

    def route_form(self) -> str:
        """The route stage's table form a launch uses now (lds: LDS
        intervals, dir: DIR-24-8, trie, bkt: bucketed intervals in L2)."""
        f = lib().cop_debug_route_form
        f.restype = c_int
        f.argtypes = [c_void_p]
        return self.ROUTE_FORMS[_check(f(self.handle), self, "route_form")]

    LAUNCH_FORMS = {0: "off", **ROUTE_FORMS}

    def launch_forms(self):
        """(firewall form, route form, dynamic LDS bytes) of the context's
        most recent one-shot launch, as the LDS budget ladder left them
        (cop_debug_launch_forms); None before any launch."""
        f = lib().cop_debug_launch_forms
        f.restype = c_int
        f.argtypes = [c_void_p, c_void_p]
        out = np.zeros(3, dtype=np.uint32)
        rc = f(self.handle, _ptr(out))
        if rc == -errno.ENOENT:
            return None
        _check(rc, self, "launch_forms")
        return self.LAUNCH_FORMS[int(out[0])], self.LAUNCH_FORMS[int(out[1])], int(out[2])

    LAUNCH_LAYOUTS = {0: "slots", 1: "imix", 2: "coalesced", 3: "hdr16"}

    def launch_plan(self):
        """(packet layout, packets per lane) of the same launch
        (cop_debug_launch_plan): slots = per-lane slot loads, imix,
        coalesced, hdr16 = packed 16- or 12-byte records; None before any
        launch."""
        f = lib().cop_debug_launch_plan
        f.restype = c_int
        f.argtypes = [c_void_p, c_void_p]
        out = np.zeros(2, dtype=np.uint32)
        rc = f(self.handle, _ptr(out))
        if rc == -errno.ENOENT:
            return None
        _check(rc, self, "launch_plan")
        return self.LAUNCH_LAYOUTS[int(out[0])], int(out[1])

    def lookup_form(self, stage: int) -> str:
        """The table form lookup_bulk uses for a stage now (ROUTE_FORMS names;
        "dir-packed": DIR-24-8 with packed tbl8 groups)."""
        f = lib().cop_debug_lookup_form
        f.restype = c_int
        f.argtypes = [c_void_p, c_uint32]
        v = _check(f(self.handle, stage), self, "lookup_form")
        return self.ROUTE_FORMS[v & 0xF] + ("-packed" if v & 0x10 else "")

    def lookup_bulk(self, stage: int, ips_buf, n: int, out_buf):
        """cop_lookup_bulk: n addresses at ips_buf (DeviceBuffer or device
        address) through the stage's table into out_buf (may be ips_buf).
        Asynchronous: the words are valid after sync()."""
        def addr(x):
            return x.addr if isinstance(x, DeviceBuffer) else int(x)
        _check(lib().cop_lookup_bulk(self.handle, stage, c_void_p(addr(ips_buf)), n, c_void_p(addr(out_buf))), self,
               "lookup_bulk")

    def lookup_bulk_host(self, stage: int, ips: np.ndarray) -> np.ndarray:
        """cop_lookup_bulk_host: host addresses in, their words out (synchronous)."""
        ips = np.ascontiguousarray(ips, dtype=np.uint32)
        out = np.zeros(len(ips), dtype=np.uint32)
        _check(lib().cop_lookup_bulk_host(self.handle, stage, _ptr(ips), len(ips), _ptr(out)), self, "lookup_bulk_host")
        return out

    def lookup_audit(self, stage: int, table: LpmTable, bad_cap: int = 0):
        """cop_lookup_audit: (report dict, mismatching addresses (at most
        bad_cap, ascending)) of the stage's device image against `table`."""
        rep = AuditReport()
        bad = np.zeros(max(bad_cap, 1), dtype=np.uint32)
        _check(lib().cop_lookup_audit(self.handle, stage, table.handle, byref(rep), _ptr(bad) if bad_cap else None,
                                      bad_cap), self, "lookup_audit")
        return rep.as_dict(), bad[: rep.n_bad]

    def set_routing_table(self, rt: np.ndarray):
        rt = np.ascontiguousarray(rt, dtype=np.uint16)
        assert rt.size == 65536
        _check(lib().cop_set_routing_table(self.handle, _ptr(rt)), self, "set_routing_table")

    def load_fw_rules_file(self, path, max_rules=1024, number_tbl8s=24, stop_at_first_error=True):
        cfg = LpmConfig(max_rules, number_tbl8s, LPM_STOP_AT_FIRST_ERROR if stop_at_first_error else 0)
        rep = LpmReport()
        _check(lib().cop_load_fw_rules_file(self.handle, path.encode(), byref(cfg), byref(rep)), self,
               "load_fw_rules_file")
        return rep

    def _update(self, fn, what, *args) -> dict:
        rep = UpdateReport()
        _check(fn(self.handle, *args, byref(rep)), self, what)
        return rep.as_dict()

    def update_fw_table(self, t: LpmTable) -> dict:
        """Bring the firewall stage to t's current rules (cop_update_fw_table):
        stream-ordered, no sync needed; returns the update report."""
        return self._update(lib().cop_update_fw_table, "update_fw_table", t.handle)

    def update_route_lpm(self, t: LpmTable) -> dict:
        return self._update(lib().cop_update_route_lpm, "update_route_lpm", t.handle)

    def update_fw_rules_file(self, t: LpmTable, path: str) -> dict:
        """Make t (and the firewall stage) hold what the edited rules file holds."""
        rep = self._update(lib().cop_update_fw_rules_file, "update_fw_rules_file", t.handle, path.encode())
        t._refresh()
        return rep

    def replace_fw_table(self, t: LpmTable) -> dict:
        """The firewall stage takes table t, whatever it held
        (cop_replace_fw_table): painted on the device in stream order, no
        sync needed; returns the update report."""
        return self._update(lib().cop_replace_fw_table, "replace_fw_table", t.handle)

    def replace_route_lpm(self, t: LpmTable) -> dict:
        return self._update(lib().cop_replace_route_lpm, "replace_route_lpm", t.handle)

    def debug_paint(self, starts: np.ndarray, entries: np.ndarray, ext24: np.ndarray, tbl24: DeviceBuffer,
                    tbl8: DeviceBuffer, cap_groups: int):
        """The paint kernel alone on two caller buffers (tests): tbl24 of 2^24
        entries, tbl8 of at least cap_groups * 256."""
        starts = np.ascontiguousarray(starts, dtype=np.uint32)
        entries = np.ascontiguousarray(entries, dtype=np.uint32)
        ext24 = np.ascontiguousarray(ext24, dtype=np.uint32)
        assert len(starts) == len(entries) and tbl24.nbytes >= 4 << 24 and tbl8.nbytes >= cap_groups * 1024
        f = lib().cop_debug_paint
        f.restype = c_int
        f.argtypes = [c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p, c_void_p, c_uint32]
        _check(f(self.handle, _ptr(starts), _ptr(entries), len(starts), _ptr(ext24) if len(ext24) else None, len(ext24),
                 tbl24.ptr, tbl8.ptr, cap_groups), self, "debug_paint")

    def debug_patch(self, tbl24: DeviceBuffer, tbl8: DeviceBuffer, recs: np.ndarray) -> int:
        """The patch kernel alone on two caller buffers (tests); returns the
        records sent after cutting long runs."""
        recs = np.ascontiguousarray(recs, dtype=PATCH_REC_DT)
        f = lib().cop_debug_patch
        f.restype = c_int
        f.argtypes = [c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p, c_uint32]
        return _check(f(self.handle, tbl24.ptr, tbl24.nbytes // 4, tbl8.ptr, tbl8.nbytes // 4, _ptr(recs), len(recs)),
                      self, "debug_patch")

    def alloc(self, nbytes, flags: int = 0) -> DeviceBuffer:
        """HBM (flags: ALLOC_UNCACHED / ALLOC_FINEGRAINED, cop_dev_alloc_ex)."""
        return DeviceBuffer(self, nbytes, flags)

    def pmd_start(self, ring, flags: int = 0) -> "Pmd":
        """Start the poll-mode (persistent) kernel serving `ring` (or a list
        of rings: one kernel serving each; PMD_VARIABLE_N in flags)."""
        return Pmd(self, ring, flags)

    def submit(self, batches):
        arr = (Batch * len(batches))(*batches)
        _check(lib().cop_submit(self.handle, arr, len(batches)), self, "submit")

    def tx_gather(self, batches, tx):
        """cop_tx_gather: the frames of the batches' forward lists (as they
        are in device memory once everything queued so far has run) packed
        into the tx bursts of `tx` (one TxDesc per batch, make_tx).
        Asynchronous: valid after sync(); synchronous beside a poll-mode kernel."""
        assert len(batches) == len(tx)
        arr, tarr = (Batch * len(batches))(*batches), (TxDesc * len(tx))(*tx)
        _check(lib().cop_tx_gather(self.handle, arr, tarr, len(batches)), self, "tx_gather")

    def submit_tx(self, batches, tx):
        """cop_submit_tx: submit(batches), then their tx gather on the same lane."""
        assert len(batches) == len(tx)
        arr, tarr = (Batch * len(batches))(*batches), (TxDesc * len(tx))(*tx)
        _check(lib().cop_submit_tx(self.handle, arr, tarr, len(batches)), self, "submit_tx")

    def sketch(self, rows: int = 4, log2_cols: int = 14, key: int = SKETCH_KEY_SRC, key_depth: int = 32,
               seed: int = 0) -> "Sketch":
        """cop_sketch_create: a count-min sketch of rows << log2_cols u64 counters on this context."""
        return Sketch(self, sketch_config(rows, log2_cols, key, key_depth, seed))

    def neigh(self, n_entries: int) -> "Neigh":
        """cop_neigh_create: a neighbour table of n_entries entries on this context, all invalid."""
        return Neigh(self, n_entries)

    def acl(self, table: "AclTable", flags: int = 0) -> "Acl":
        """cop_acl_create: the built table's image on this context (ACL_COUNTERS: a hit counter per rule)."""
        return Acl(self, table, flags)

    def fwd_check(self, neigh: "Neigh", cfg: "FwdConfig", batches, descs):
        """cop_fwd_check: the batches' forward lists filtered into the lists of `descs` (one FwdCheckDesc per
        batch, make_fwd_check). Asynchronous: valid after sync(); synchronous beside a poll-mode kernel."""
        assert len(batches) == len(descs)
        arr, darr = (Batch * len(batches))(*batches), (FwdCheckDesc * len(descs))(*descs)
        _check(lib().cop_fwd_check(self.handle, neigh.handle, byref(cfg), arr, darr, len(batches)), self, "fwd_check")

    def fwd_rewrite(self, neigh: "Neigh", cfg: "FwdConfig", batches, tx, rw):
        """cop_fwd_rewrite: the frames cop_tx_gather of the same batches and tx left, rewritten in place
        (one FwdRwDesc per batch, make_fwd_rw)."""
        assert len(batches) == len(tx) == len(rw)
        arr, tarr, rarr = (Batch * len(batches))(*batches), (TxDesc * len(tx))(*tx), (FwdRwDesc * len(rw))(*rw)
        _check(lib().cop_fwd_rewrite(self.handle, neigh.handle, byref(cfg), arr, tarr, rarr, len(batches)), self,
               "fwd_rewrite")

    def aead_seal(self, key: "AeadKey", bursts):
        """cop_aead_seal: ChaCha20-Poly1305 over the frames of the bursts (make_aead_burst) in place,
        tags written. Asynchronous: valid after sync(); synchronous beside a poll-mode kernel."""
        arr = (AeadBurst * len(bursts))(*bursts)
        _check(lib().cop_aead_seal(self.handle, byref(key), arr, len(bursts)), self, "aead_seal")

    def aead_open(self, key: "AeadKey", bursts):
        """cop_aead_open: tags checked, ok[] written, authentic frames decrypted in place."""
        arr = (AeadBurst * len(bursts))(*bursts)
        _check(lib().cop_aead_open(self.handle, byref(key), arr, len(bursts)), self, "aead_open")

    def poly1305_bulk(self, burst: "AeadBurst", otk):
        """cop_poly1305_bulk: tags[k] = Poly1305(otk[k], frame k); otk a DeviceBuffer or address."""
        a = otk.addr if isinstance(otk, DeviceBuffer) else otk
        _check(lib().cop_poly1305_bulk(self.handle, byref(burst), a), self, "poly1305_bulk")

    def submit_ring(self, ring: BatchRing, first_slot: int, count: int):
        _check(lib().cop_submit_ring(self.handle, byref(ring), first_slot, count), self, "submit_ring")

    def sync(self):
        _check(lib().cop_sync(self.handle), self, "sync")

    def counters(self, reset=False) -> dict:
        c = np.zeros(16, dtype=np.uint64)
        _check(lib().cop_counters_read(self.handle, _ptr(c), 1 if reset else 0), self, "counters")
        return {k: int(c[i]) for i, k in enumerate(COUNTER_NAMES)}

    def counters_device_ptr(self) -> int:
        return lib().cop_counters_device_ptr(self.handle)

    def port_stats(self, reset=False) -> list:
        """Per-port coprocessor_stats (CFG_PORT_STATS), synchronous."""
        arr = (PortStats * MAX_DEMUX_PORTS)()
        n = _check(lib().cop_port_stats_read(self.handle, arr, MAX_DEMUX_PORTS, 1 if reset else 0), self,
                   "port_stats")
        return [arr[i].as_dict() for i in range(n)]

    def snapshot(self, reset=False, ports=0):
        """Live counters (+ per-port stats) without waiting for submitted work."""
        c = np.zeros(16, dtype=np.uint64)
        arr = (PortStats * MAX_DEMUX_PORTS)()
        _check(lib().cop_counters_snapshot(self.handle, _ptr(c), arr, ports, 1 if reset else 0), self, "snapshot")
        return {k: int(c[i]) for i, k in enumerate(COUNTER_NAMES)}, [arr[i].as_dict() for i in range(ports)]

    def rule_counters(self, reset=False) -> np.ndarray:
        """Per-rule FW hit counters (CFG_RULE_COUNTERS), indexed by rule id."""
        n = _check(lib().cop_rule_counters_read(self.handle, None, 0, 0), self, "rule_counters")
        out = np.zeros(n, dtype=np.uint64)
        _check(lib().cop_rule_counters_read(self.handle, _ptr(out), n, 1 if reset else 0), self, "rule_counters")
        return out

    def coll_init(self, uid: bytes, rank: int, nranks: int):
        buf = (c_uint8 * COLL_ID_BYTES).from_buffer_copy(uid)
        _check(lib().cop_coll_init(self.handle, buf, rank, nranks), self, "coll_init")

    def coll_reduce_counters(self, reset=False, with_rules=True):
        """RCCL all-reduce of counters (+ per-rule counters) over the ranks."""
        c = np.zeros(16, dtype=np.uint64)
        n = 0
        if with_rules and (self.cfg.flags & CFG_RULE_COUNTERS):
            n = _check(lib().cop_rule_counters_read(self.handle, None, 0, 0), self, "rule_counters")
        hits = np.zeros(max(n, 1), dtype=np.uint64)
        _check(lib().cop_coll_reduce_counters(self.handle, _ptr(c), _ptr(hits), n, 1 if reset else 0), self,
               "coll_reduce_counters")
        return {k: int(c[i]) for i, k in enumerate(COUNTER_NAMES)}, hits[:n]

    def process_host(self, pkts: np.ndarray, n: int, stride: int = 64):
        """End-to-end: host packet memory -> pinned gather -> H2D -> kernel -> D2H."""
        base = pkts.ctypes.data
        ptrs = (c_void_p * n)(*[base + i * stride for i in range(n)])
        res = np.zeros(n, dtype=RESULT_DT)
        fwd = np.zeros(max(n, 1), dtype=np.uint32)
        cnt = c_uint32(0)
        _check(lib().cop_process_host(self.handle, ptrs, n, _ptr(res), _ptr(fwd), byref(cnt)), self,
               "process_host")
        return res, fwd[: cnt.value]

    def set_host_threads(self, n: int):
        _check(lib().cop_set_host_threads(self.handle, n), self, "set_host_threads")

    def process_host_stream(self, ptrs: np.ndarray, batch: int, out: np.ndarray | None = None) -> np.ndarray:
        """Streaming end-to-end path over host packet addresses (u64 array).
        out: a RESULT_DT array of len(ptrs) to fill (timed loops reuse one)."""
        ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
        if out is not None:
            assert out.dtype == RESULT_DT and len(out) == len(ptrs) and out.flags.c_contiguous
            res = out
        else:
            res = np.zeros(len(ptrs), dtype=RESULT_DT)
        _check(lib().cop_process_host_stream(self.handle, _ptr(ptrs), len(ptrs), batch, _ptr(res)), self,
               "process_host_stream")
        return res

    def timer_start(self):
        _check(lib().cop_timer_start(self.handle), self, "timer_start")

    def timer_stop(self) -> float:
        ms = c_double(0)
        _check(lib().cop_timer_stop(self.handle, byref(ms)), self, "timer_stop")
        return ms.value

    def launch_timing(self, enable=True):
        _check(lib().cop_launch_timing(self.handle, 1 if enable else 0), self, "launch_timing")

    def launch_timing_read(self, reset=True):
        ms = c_double(0)
        n = c_uint64(0)
        _check(lib().cop_launch_timing_read(self.handle, byref(ms), byref(n), 1 if reset else 0), self,
               "launch_timing_read")
        return ms.value, n.value


PMD_VARIABLE_N = 1
PMD_SYS_ACQUIRE = 2     # acquire on every tile
PMD_STATIC_SLOTS = 4    # slots written once before the start: plain loads (default: coherent loads once the ring wraps)
PMD_DYNAMIC_TILES = 8   # tiles claimed from tickets, the next tile's loads issued early (segmented lists)


class Pmd:
    """A poll-mode kernel serving one batch ring (cop_pmd_*): post(count)
    hands the next `count` slots to the running kernel (batch sequence
    numbers continue across posts; batch b sits in slot b % n_slots),
    wait(seq) blocks until batches < seq have completed. With a list of
    rings (cop_pmd_start_rings), one kernel serves them all: ring r is
    posted and waited with post_ring / post_batch / wait_ring."""

    def __init__(self, ctx: "Context", ring, flags: int = 0):
        self.ctx = ctx
        self.handle = c_void_p()
        if isinstance(ring, (list, tuple)):
            arr = (BatchRing * len(ring))(*ring)
            self.ring = arr   # keep the descriptors alive
            self.n_rings = len(ring)
            _check(lib().cop_pmd_start_rings(ctx.handle, arr, len(ring), flags, byref(self.handle)), ctx,
                   "pmd_start_rings")
        else:
            self.ring = ring   # keep the descriptor alive
            self.n_rings = 1
            if flags:
                arr = (BatchRing * 1)(ring)
                self.ring = arr
                _check(lib().cop_pmd_start_rings(ctx.handle, arr, 1, flags, byref(self.handle)), ctx,
                       "pmd_start_rings")
            else:
                _check(lib().cop_pmd_start(ctx.handle, byref(ring), byref(self.handle)), ctx, "pmd_start")
        if not hasattr(ctx, "_pmds"):
            ctx._pmds = []
        ctx._pmds.append(self)
        # bound once: these sit inside timed regions (a lookup per call costs
        # a measurable part of a 30 us post)
        L = lib()
        self._post, self._wait, self._run = L.cop_pmd_post, L.cop_pmd_wait, L.cop_pmd_run
        self._run_timed = L.cop_pmd_run_timed
        self._t = (c_uint64(0), c_uint64(0))
        self._tp = (byref(self._t[0]), byref(self._t[1]))
        self._n_posted = 0   # every post goes through this object

    def post(self, count: int):
        _check(self._post(self.handle, count), self.ctx, "pmd_post")
        self._n_posted += count

    def wait(self, seq: int | None = None):
        rc = self._wait(self.handle, self._n_posted if seq is None else seq)
        if rc < 0:
            _check(rc, self.ctx, "pmd_wait")

    def run(self, count: int):
        """Post `count` batches and wait for all of them (one C call)."""
        rc = self._run(self.handle, count)
        if rc < 0:
            _check(rc, self.ctx, "pmd_run")
        self._n_posted += count

    def run_timed(self, count: int):
        """run(count), returning (t_post_ns, t_done_ns): CLOCK_MONOTONIC taken
        inside the library just before the first post and just after the
        last completion (cop_pmd_run_timed)."""
        rc = self._run_timed(self.handle, count, *self._tp)
        if rc < 0:
            _check(rc, self.ctx, "pmd_run_timed")
        self._n_posted += count
        return self._t[0].value, self._t[1].value

    @property
    def posted(self) -> int:
        return int(lib().cop_pmd_posted(self.handle))

    def post_ring(self, ring: int, count: int):
        _check(lib().cop_pmd_post_ring(self.handle, ring, count), self.ctx, "pmd_post_ring")

    def post_batch(self, ring: int, n: int):
        """One batch of n packets (PMD_VARIABLE_N) to `ring`."""
        _check(lib().cop_pmd_post_batch(self.handle, ring, n), self.ctx, "pmd_post_batch")

    def wait_ring(self, ring: int, seq: int | None = None):
        if seq is None:
            seq = int(lib().cop_pmd_posted_ring(self.handle, ring))
        _check(lib().cop_pmd_wait_ring(self.handle, ring, seq), self.ctx, "pmd_wait_ring")

    def posted_ring(self, ring: int) -> int:
        return int(lib().cop_pmd_posted_ring(self.handle, ring))

    def completed_ring(self, ring: int) -> int:
        return int(lib().cop_pmd_completed_ring(self.handle, ring))

    def info(self) -> dict:
        i = PmdInfo()
        _check(lib().cop_pmd_info(self.handle, byref(i)), self.ctx, "pmd_info")
        d = {k: getattr(i, k) for k, _ in PmdInfo._fields_}
        k = d["kernel"]
        # the instantiation's template arguments, as rocprofv3 names the kernel
        d["kernel_name"] = (f"cop_pmd<{k & 15}, {(k >> 4) & 15}, {(k >> 8) & 15}, {d['packets_per_tile'] // 256}, "
                            f"{'true' if (k >> 12) & 1 else 'false'}>")
        return d

    def launch_forms(self):
        """(firewall form, route form, dynamic LDS bytes) of this kernel
        (cop_debug_pmd_forms; the forms are also in info()["kernel"])."""
        f = lib().cop_debug_pmd_forms
        f.restype = c_int
        f.argtypes = [c_void_p, c_void_p]
        out = np.zeros(3, dtype=np.uint32)
        _check(f(self.handle, _ptr(out)), self.ctx, "pmd_forms")
        return Context.LAUNCH_FORMS[int(out[0])], Context.LAUNCH_FORMS[int(out[1])], int(out[2])

    def stop(self):
        if self.handle and self.handle.value:
            h, self.handle = self.handle, c_void_p()
            if self in getattr(self.ctx, "_pmds", []):
                self.ctx._pmds.remove(self)
            _check(lib().cop_pmd_stop(h), self.ctx, "pmd_stop")

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.stop()


def make_ring(pkts, n_slots: int, n: int, results, pkts_slot_bytes: int, results_slot: int = 0,
              fwd_idx=None, fwd_slot: int = 0, fwd_count=None, stride: int = 64, offsets=None,
              offsets_slot_words: int = 0, data_off: int = 0) -> BatchRing:
    def addr(x):
        if x is None:
            return None
        return x.addr if isinstance(x, DeviceBuffer) else int(x)
    r = BatchRing()
    r.pkts, r.offsets, r.results = addr(pkts), addr(offsets), addr(results)
    r.fwd_idx, r.fwd_count = addr(fwd_idx), addr(fwd_count)
    r.pkts_slot_bytes, r.offsets_slot_words = pkts_slot_bytes, offsets_slot_words
    r.results_slot = results_slot or n
    r.fwd_slot = fwd_slot or n
    r.n_slots, r.n, r.stride, r.data_off = n_slots, n, stride, data_off
    # the ring holds device addresses only: keep the buffers it was made from
    # alive as long as the ring (a collected DeviceBuffer frees its memory,
    # and a kernel writing through the stale address would fault the GPU)
    r._keep = tuple(x for x in (pkts, offsets, results, fwd_idx, fwd_count) if isinstance(x, DeviceBuffer))
    return r


def make_batch(pkts: DeviceBuffer | int, n: int, results: DeviceBuffer | int, stride: int = 64,
               offsets: DeviceBuffer | int | None = None, fwd_idx=None, fwd_count=None,
               data_off: int = 0, pkts_offset: int = 0, results_offset: int = 0) -> Batch:
    def addr(x, off=0):
        if x is None:
            return None
        return (x.addr if isinstance(x, DeviceBuffer) else int(x)) + off
    b = Batch()
    b.pkts = addr(pkts, pkts_offset)
    b.offsets = addr(offsets)
    b.n = n
    b.stride = stride
    b.data_off = data_off
    b.results = addr(results, results_offset)
    b.fwd_idx = addr(fwd_idx)
    b.fwd_count = addr(fwd_count)
    b._keep = tuple(x for x in (pkts, offsets, results, fwd_idx, fwd_count) if isinstance(x, DeviceBuffer))
    return b


def sketch_config(rows: int = 4, log2_cols: int = 14, key: int = SKETCH_KEY_SRC, key_depth: int = 32,
                  seed: int = 0) -> SketchConfig:
    cfg = SketchConfig()
    cfg.rows, cfg.log2_cols, cfg.key, cfg.key_depth, cfg.seed = rows, log2_cols, key, key_depth, seed
    return cfg


class Sketch:
    """A context's count-min sketch (cop_sketch_*). Every call but read() is
    asynchronous (valid after ctx.sync()); synchronous beside a poll-mode kernel."""

    def __init__(self, ctx: "Context", cfg: SketchConfig):
        self.ctx, self.cfg, self.handle = ctx, cfg, c_void_p()
        _check(lib().cop_sketch_create(ctx.handle, byref(cfg), byref(self.handle)), ctx, "sketch_create")
        self.words = cfg.rows << cfg.log2_cols

    def destroy(self):
        if self.handle:
            h, self.handle = self.handle, c_void_p()
            _check(lib().cop_sketch_destroy(self.ctx.handle, h), self.ctx, "sketch_destroy")

    def update(self, batches, verdict_mask: int = 0):
        arr = (Batch * len(batches))(*batches)
        _check(lib().cop_sketch_update(self.ctx.handle, self.handle, arr, len(batches), verdict_mask), self.ctx,
               "sketch_update")

    def query(self, ips, n: int, out):
        """ips: n u32 device words, out: n u64 device words (DeviceBuffer or address)."""
        a = lambda x: x.addr if isinstance(x, DeviceBuffer) else x
        _check(lib().cop_sketch_query(self.ctx.handle, self.handle, a(ips), n, a(out)), self.ctx, "sketch_query")

    def police(self, batches, pol):
        assert len(batches) == len(pol)
        arr, parr = (Batch * len(batches))(*batches), (PoliceDesc * len(pol))(*pol)
        _check(lib().cop_sketch_police(self.ctx.handle, self.handle, arr, parr, len(batches)), self.ctx,
               "sketch_police")

    def decay(self, shift: int):
        _check(lib().cop_sketch_decay(self.ctx.handle, self.handle, shift), self.ctx, "sketch_decay")

    def read(self, cap_words: int | None = None) -> np.ndarray:
        """cop_sketch_read: the counters, rows x cols (synchronous)."""
        cap = self.words if cap_words is None else cap_words
        out = np.zeros(max(cap, 1), dtype=np.uint64)
        rc = lib().cop_sketch_read(self.ctx.handle, self.handle, out.ctypes.data, cap)
        if rc < 0:
            _check(rc, self.ctx, "sketch_read")
        return out[:rc].reshape(self.cfg.rows, -1)

    def device_ptr(self):
        """(device address of the counters, words)."""
        p, w = c_void_p(), c_uint64()
        _check(lib().cop_sketch_device_ptr(self.ctx.handle, self.handle, byref(p), byref(w)), self.ctx,
               "sketch_device_ptr")
        return p.value, w.value


def make_police(threshold: int, out_idx, out_count, status) -> PoliceDesc:
    """A batch's cop_police_desc (DeviceBuffer, address or None each)."""
    a = lambda x: x.addr if isinstance(x, DeviceBuffer) else x
    p = PoliceDesc()
    p.threshold, p.out_idx, p.out_count, p.status = threshold, a(out_idx), a(out_count), a(status)
    p._keep = tuple(x for x in (out_idx, out_count, status) if isinstance(x, DeviceBuffer))
    return p


def sketch_params(cfg: SketchConfig):
    """cop_sketch_params: (a, b), 4 u32 each; None on -EINVAL."""
    a, b = (c_uint32 * 4)(), (c_uint32 * 4)()
    if lib().cop_sketch_params(byref(cfg), a, b):
        return None
    return np.array(a[:], dtype=np.uint32), np.array(b[:], dtype=np.uint32)


def sketch_update_host(cfg: SketchConfig, counters: np.ndarray, batches, verdict_mask: int = 0, max_batch: int = 0) -> int:
    """cop_sketch_update_host over host memory (every pointer a host address). Returns the C code."""
    arr = (Batch * len(batches))(*batches)
    return lib().cop_sketch_update_host(byref(cfg), counters.ctypes.data, arr, len(batches), verdict_mask, max_batch)


def sketch_query_host(cfg: SketchConfig, counters: np.ndarray, ips: np.ndarray, out: np.ndarray, n=None) -> int:
    return lib().cop_sketch_query_host(byref(cfg), counters.ctypes.data, ips.ctypes.data,
                                       len(ips) if n is None else n, out.ctypes.data)


def sketch_police_host(cfg: SketchConfig, counters: np.ndarray, batches, pol, n_lists: int = 1, seg: bool = False,
                       max_batch: int = 0) -> int:
    assert len(batches) == len(pol)
    arr, parr = (Batch * len(batches))(*batches), (PoliceDesc * len(pol))(*pol)
    return lib().cop_sketch_police_host(byref(cfg), counters.ctypes.data, arr, parr, len(batches), n_lists,
                                        1 if seg else 0, max_batch)


def fwd_config(flags: int = 0, miss_nh: int = FWD_NO_NH) -> FwdConfig:
    cfg = FwdConfig()
    cfg.flags, cfg.miss_nh = flags, miss_nh
    return cfg


class Neigh:
    """A context's neighbour table (cop_neigh_*): 16-byte entries (NEIGH_DT) indexed by next hop."""

    def __init__(self, ctx: "Context", n_entries: int):
        self.ctx, self.handle, self.n_entries = ctx, c_void_p(), n_entries
        _check(lib().cop_neigh_create(ctx.handle, n_entries, byref(self.handle)), ctx, "neigh_create")

    def set(self, first: int, entries: np.ndarray, count: int | None = None):
        """cop_neigh_set: entries (NEIGH_DT) to first .. ; synchronous."""
        a = None if entries is None else np.ascontiguousarray(entries, dtype=NEIGH_DT)
        n = (0 if a is None else len(a)) if count is None else count
        _check(lib().cop_neigh_set(self.ctx.handle, self.handle, first, n, None if a is None else a.ctypes.data),
               self.ctx, "neigh_set")

    def destroy(self):
        if self.handle:
            h, self.handle = self.handle, c_void_p()
            _check(lib().cop_neigh_destroy(self.ctx.handle, h), self.ctx, "neigh_destroy")

    def device_ptr(self):
        """(device address of the entries, n_entries)."""
        p, n = c_void_p(), c_uint32()
        _check(lib().cop_neigh_device_ptr(self.ctx.handle, self.handle, byref(p), byref(n)), self.ctx,
               "neigh_device_ptr")
        return p.value, n.value


def make_fwd_check(out_idx, out_count, status, lens=None, exc_idx=None, exc_count=None) -> FwdCheckDesc:
    """A batch's cop_fwd_check_desc (DeviceBuffer, address or None each)."""
    a = lambda x: x.addr if isinstance(x, DeviceBuffer) else x
    d = FwdCheckDesc()
    d.lens, d.out_idx, d.out_count, d.exc_idx, d.exc_count, d.status = (a(x) for x in (lens, out_idx, out_count, exc_idx,
                                                                                       exc_count, status))
    d._keep = tuple(x for x in (lens, out_idx, out_count, exc_idx, exc_count, status) if isinstance(x, DeviceBuffer))
    return d


def make_fwd_rw(status, port=None) -> FwdRwDesc:
    """A batch's cop_fwd_rw_desc: status (and port) one per burst, or a single one."""
    a = lambda x: x.addr if isinstance(x, DeviceBuffer) else x
    st = status if isinstance(status, (list, tuple)) else [status]
    pt = port if isinstance(port, (list, tuple)) else [port] * len(st)
    d = FwdRwDesc()
    for q, (s_, p_) in enumerate(zip(st, pt)):
        d.status[q], d.port[q] = a(s_), a(p_)
    d._keep = tuple(x for x in list(st) + list(pt) if isinstance(x, DeviceBuffer))
    return d


def fwd_check_host(entries: np.ndarray, cfg: FwdConfig, batches, descs, n_lists: int = 1, seg: bool = False,
                   max_batch: int = 0, n_entries: int | None = None) -> int:
    """cop_fwd_check_host over host memory (entries: NEIGH_DT; every pointer a host address). Returns the C code."""
    assert len(batches) == len(descs)
    arr, darr = (Batch * len(batches))(*batches), (FwdCheckDesc * len(descs))(*descs)
    return lib().cop_fwd_check_host(entries.ctypes.data, len(entries) if n_entries is None else n_entries, byref(cfg),
                                    arr, darr, len(batches), n_lists, 1 if seg else 0, max_batch)


def fwd_rewrite_host(entries: np.ndarray, cfg: FwdConfig, batches, tx, rw, n_lists: int = 1, seg: bool = False,
                     max_batch: int = 0, n_entries: int | None = None) -> int:
    assert len(batches) == len(tx) == len(rw)
    arr, tarr, rarr = (Batch * len(batches))(*batches), (TxDesc * len(tx))(*tx), (FwdRwDesc * len(rw))(*rw)
    return lib().cop_fwd_rewrite_host(entries.ctypes.data, len(entries) if n_entries is None else n_entries,
                                      byref(cfg), arr, tarr, rarr, len(batches), n_lists, 1 if seg else 0, max_batch)


def ipv4_csum_host(hdr) -> int:
    """cop_ipv4_csum_host: the checksum of a 20-byte IPv4 header (bytes 10..11 taken as zero)."""
    a = np.ascontiguousarray(hdr, dtype=np.uint8)
    assert a.size == 20
    return int(lib().cop_ipv4_csum_host(a.ctypes.data))


def acl_rules(n: int) -> np.ndarray:
    """n zeroed rules (ACL_RULE_DT) that match everything: depth 0, any protocol, ports 0..65535."""
    r = np.zeros(n, dtype=ACL_RULE_DT)
    r["sport_hi"] = r["dport_hi"] = 0xFFFF
    return r


class AclTable:
    """A built ACL image (cop_acl_build; host only). Raises CopError with .report set on a bad rule set."""

    def __init__(self, rules: np.ndarray, n: int | None = None):
        rules = np.ascontiguousarray(rules, dtype=ACL_RULE_DT)
        self.handle, self.report = c_void_p(), AclReport()
        rc = lib().cop_acl_build(rules.ctypes.data if len(rules) else None, len(rules) if n is None else n,
                                 byref(self.handle), byref(self.report))
        if rc < 0:
            e = CopError(rc, "acl_build")
            e.report = self.report
            raise e
        self.n_rules = self.report.n_rules

    def free(self):
        if self.handle:
            h, self.handle = self.handle, c_void_p()
            lib().cop_acl_free(h)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def match(self, keys: np.ndarray) -> np.ndarray:
        """cop_acl_match_host: the word of every key (ACL_KEY_DT)."""
        keys = np.ascontiguousarray(keys, dtype=ACL_KEY_DT)
        out = np.zeros(len(keys), dtype=np.uint32)
        rc = lib().cop_acl_match_host(self.handle, keys.ctypes.data, len(keys), out.ctypes.data)
        if rc < 0:
            raise CopError(rc, "acl_match_host")
        return out


class Acl:
    """A context's ACL (cop_acl_*). classify() and filter() are asynchronous (valid after
    ctx.sync()); synchronous beside a poll-mode kernel."""

    def __init__(self, ctx: "Context", table: AclTable, flags: int = 0):
        self.ctx, self.handle, self.flags = ctx, c_void_p(), flags
        _check(lib().cop_acl_create(ctx.handle, table.handle, flags, byref(self.handle)), ctx, "acl_create")
        self.n_rules = table.n_rules

    def set(self, table: AclTable):
        _check(lib().cop_acl_set(self.ctx.handle, self.handle, table.handle), self.ctx, "acl_set")
        self.n_rules = table.n_rules

    def destroy(self):
        if self.handle:
            h, self.handle = self.handle, c_void_p()
            _check(lib().cop_acl_destroy(self.ctx.handle, h), self.ctx, "acl_destroy")

    def classify(self, batches, descs):
        assert len(batches) == len(descs)
        arr, darr = (Batch * len(batches))(*batches), (AclDesc * len(descs))(*descs)
        _check(lib().cop_acl_classify(self.ctx.handle, self.handle, arr, darr, len(batches)), self.ctx, "acl_classify")

    def filter(self, batches, descs):
        assert len(batches) == len(descs)
        arr, darr = (Batch * len(batches))(*batches), (AclDesc * len(descs))(*descs)
        _check(lib().cop_acl_filter(self.ctx.handle, self.handle, arr, darr, len(batches)), self.ctx, "acl_filter")

    def counters(self, reset: bool = False, cap: int | None = None) -> np.ndarray:
        """cop_acl_counters_read: one u64 per rule index (synchronous)."""
        cap = self.n_rules if cap is None else cap
        out = np.zeros(max(cap, 1), dtype=np.uint64)
        rc = _check(lib().cop_acl_counters_read(self.ctx.handle, self.handle, out.ctypes.data, cap, 1 if reset else 0),
                    self.ctx, "acl_counters_read")
        return out[:min(cap, rc)]

    def device_ptr(self):
        """(device address of the image, its bytes, device address of the counters or None, n_rules)."""
        img, nbytes, ctr, n = c_void_p(), c_uint64(), c_void_p(), c_uint32()
        _check(lib().cop_acl_device_ptr(self.ctx.handle, self.handle, byref(img), byref(nbytes), byref(ctr), byref(n)),
               self.ctx, "acl_device_ptr")
        return img.value, nbytes.value, ctr.value, n.value


def make_acl_desc(words=None, out_idx=None, out_count=None, status=None) -> AclDesc:
    """A batch's cop_acl_desc (DeviceBuffer, address or None each): words for classify, the rest for filter."""
    a = lambda x: x.addr if isinstance(x, DeviceBuffer) else x
    d = AclDesc()
    d.words, d.out_idx, d.out_count, d.status = a(words), a(out_idx), a(out_count), a(status)
    d._keep = tuple(x for x in (words, out_idx, out_count, status) if isinstance(x, DeviceBuffer))
    return d


def acl_classify_host(table: AclTable, batches, descs, max_batch: int = 0) -> int:
    """cop_acl_classify_host over host memory (every pointer a host address). Returns the C code."""
    assert len(batches) == len(descs)
    arr, darr = (Batch * len(batches))(*batches), (AclDesc * len(descs))(*descs)
    return lib().cop_acl_classify_host(table.handle, arr, darr, len(batches), max_batch)


def acl_filter_host(table: AclTable, counters, batches, descs, n_lists: int = 1, seg: bool = False,
                    max_batch: int = 0) -> int:
    """cop_acl_filter_host; counters: n_rules u64 or None."""
    assert len(batches) == len(descs)
    arr, darr = (Batch * len(batches))(*batches), (AclDesc * len(descs))(*descs)
    return lib().cop_acl_filter_host(table.handle, None if counters is None else counters.ctypes.data, arr, darr,
                                     len(batches), n_lists, 1 if seg else 0, max_batch)


def make_tx(out, lens=None, copy_bytes: int = 0, slot_bytes: int = 0) -> TxDesc:
    """A batch's cop_tx_desc. out: one burst, or one per vport, each a dict
    (or tuple in this order) of frames, off, len, status (DeviceBuffer, address
    or None), cap_bytes, cap_frames. Slot batches give copy_bytes (slot_bytes
    defaults to it), IMIX batches lens."""
    def addr(x):
        if x is None:
            return None
        return x.addr if isinstance(x, DeviceBuffer) else int(x)
    t = TxDesc()
    t.lens = addr(lens)
    t.copy_bytes, t.slot_bytes = copy_bytes, (slot_bytes or copy_bytes)
    bursts = out if isinstance(out, (list, tuple)) and out and isinstance(out[0], (dict, list, tuple)) else [out]
    assert 1 <= len(bursts) <= MAX_DEMUX_PORTS
    keep = [lens] if isinstance(lens, DeviceBuffer) else []
    for q, b in enumerate(bursts):
        if not isinstance(b, dict):
            b = dict(zip(("frames", "off", "len", "status", "cap_bytes", "cap_frames"), b))
        o = t.out[q]
        o.frames, o.off, o.len, o.status = (addr(b.get(k)) for k in ("frames", "off", "len", "status"))
        o.cap_bytes, o.cap_frames = int(b["cap_bytes"]), int(b["cap_frames"])
        keep += [b.get(k) for k in ("frames", "off", "len", "status") if isinstance(b.get(k), DeviceBuffer)]
    t._keep = tuple(keep)
    return t


def tx_gather_host(batches, tx, n_lists: int = 1, seg: bool = False, max_batch: int = 0) -> int:
    """cop_tx_gather_host: the gather over host memory (every pointer in the
    batches and descriptors a host address, e.g. ndarray.ctypes.data); the
    list layout explicit: n_lists lists per batch, seg for segmented lists.
    Returns the C return code (0 or -EINVAL)."""
    assert len(batches) == len(tx)
    arr, tarr = (Batch * len(batches))(*batches), (TxDesc * len(tx))(*tx)
    return lib().cop_tx_gather_host(arr, tarr, len(batches), n_lists, 1 if seg else 0, max_batch)


def aead_key(key: bytes, salt: bytes = b"\0\0\0\0") -> AeadKey:
    """A cop_aead_key: 32 key bytes, 4 salt bytes (nonce bytes 0..3)."""
    assert len(key) == 32 and len(salt) == 4
    k = AeadKey()
    k.key[:] = key
    k.salt[:] = salt
    return k


def make_aead_burst(frames, tags, status, n_frames: int, cap_bytes: int, off=None, len=None, count=None, ok=None,
                    seq_base: int = 0, slot_bytes: int = 0, frame_bytes: int = 0, aad_bytes: int = 0) -> AeadBurst:
    """A cop_aead_burst (DeviceBuffer, address or None each pointer). off / len: both or neither
    (then the slot form: frame k at k * slot_bytes, frame_bytes long)."""
    def addr(x):
        if x is None:
            return None
        return x.addr if isinstance(x, DeviceBuffer) else int(x)
    b = AeadBurst()
    b.frames, b.off, b.len, b.count = addr(frames), addr(off), addr(len), addr(count)
    b.tags, b.ok, b.status = addr(tags), addr(ok), addr(status)
    b.cap_bytes, b.seq_base, b.n_frames = cap_bytes, seq_base & 0xFFFFFFFFFFFFFFFF, n_frames
    b.slot_bytes, b.frame_bytes, b.aad_bytes = slot_bytes, frame_bytes, aad_bytes
    b._keep = tuple(x for x in (frames, off, len, count, tags, ok, status) if isinstance(x, DeviceBuffer))
    return b


def aead_seal_host(key: AeadKey, bursts) -> int:
    """cop_aead_seal_host over host memory (every pointer a host address). Returns the C code."""
    arr = (AeadBurst * len(bursts))(*bursts)
    return lib().cop_aead_seal_host(byref(key), arr, len(bursts))


def aead_open_host(key: AeadKey, bursts) -> int:
    arr = (AeadBurst * len(bursts))(*bursts)
    return lib().cop_aead_open_host(byref(key), arr, len(bursts))


def chacha20_block_host(key: bytes, counter: int, nonce: bytes) -> bytes:
    """cop_chacha20_block_host: one 64-byte ChaCha20 block."""
    assert len(key) == 32 and len(nonce) == 12
    out = ctypes.create_string_buffer(64)
    lib().cop_chacha20_block_host(key, counter, nonce, out)
    return out.raw


def poly1305_host(otk: bytes, msg: bytes) -> bytes:
    """cop_poly1305_host: the 16-byte tag of msg under the one-time key r || s."""
    assert len(otk) == 32
    out = ctypes.create_string_buffer(16)
    lib().cop_poly1305_host(otk, msg, len(msg), out)
    return out.raw
