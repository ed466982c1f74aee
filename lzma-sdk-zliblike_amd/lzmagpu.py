"""lzmagpu -- Python mirror of liblzmagpu.so (include/lzma_gpu.h) over ctypes.

The product is the C ABI; this module only binds it for the test-suite and
bench.py.  Function names and argument meaning follow the reference C API
(LzmaDec.h / LzmaLib.h / Lzma2Dec.h): ``LzmaDecode`` returns the same
``(res, status, destLen, srcLen)`` the reference returns through its
out-parameters, plus the output bytes.

There is no fallback: if lib/liblzmagpu.so is missing this module raises at
import time, and on a machine without a HIP device every decode and encode
returns SZ_ERROR_FAIL (``LzmaGpu_LastError`` says why).  Encoding (the
reference's fast path, levels 0..4): ``encode_batch``, ``LzmaEncode``,
``LzmaCompress`` and the ``LzmaEncGpu_*`` batch calls; sessions that take their
streams in pieces: ``LzmaEncSessions``, ``enc_session_*`` and the ``LzmaEnc_*``
handle drop-ins; LZMA2 and xz writing over
them: ``lzma2_encode_batch``, ``lzma2_compress``, ``xz_compress`` and the
``Lzma2Enc_*`` drop-ins.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# LZGPU_LIB may name a code-shape variant build (lib/variants/, A/B runs only)
LIB_PATH = os.environ.get("LZGPU_LIB") or os.path.join(HERE, "lib", "liblzmagpu.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(f"liblzmagpu.so not built ({LIB_PATH}); run __graft_entry__.build()")

SZ_OK, SZ_ERROR_DATA, SZ_ERROR_MEM, SZ_ERROR_UNSUPPORTED = 0, 1, 2, 4
SZ_ERROR_PARAM, SZ_ERROR_INPUT_EOF, SZ_ERROR_FAIL = 5, 6, 11
LZMA_FINISH_ANY, LZMA_FINISH_END = 0, 1
KIND_LZMA, KIND_LZMA2 = 0, 1

_lib = ctypes.CDLL(LIB_PATH)
_sp = ctypes.POINTER(ctypes.c_size_t)
_ip = ctypes.POINTER(ctypes.c_int)


class ISzAlloc(ctypes.Structure):
    _fields_ = [("Alloc", ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)),
                ("Free", ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p))]


class CLzmaProps(ctypes.Structure):
    _fields_ = [("lc", ctypes.c_uint), ("lp", ctypes.c_uint), ("pb", ctypes.c_uint),
                ("dicSize", ctypes.c_uint32)]


class CLzmaDec(ctypes.Structure):
    """Public layout of LzmaDec.h:50-69."""
    _fields_ = [("prop", CLzmaProps), ("probs", ctypes.c_void_p), ("dic", ctypes.c_void_p),
                ("buf", ctypes.c_void_p), ("range", ctypes.c_uint32), ("code", ctypes.c_uint32),
                ("dicPos", ctypes.c_size_t), ("dicBufSize", ctypes.c_size_t),
                ("processedPos", ctypes.c_uint32), ("checkDicSize", ctypes.c_uint32),
                ("state", ctypes.c_uint), ("reps", ctypes.c_uint32 * 4),
                ("remainLen", ctypes.c_uint), ("needFlush", ctypes.c_int),
                ("needInitState", ctypes.c_int), ("numProbs", ctypes.c_uint32),
                ("tempBufSize", ctypes.c_uint), ("tempBuf", ctypes.c_ubyte * 20)]


class CLzma2Dec(ctypes.Structure):
    _fields_ = [("decoder", CLzmaDec), ("packSize", ctypes.c_uint32),
                ("unpackSize", ctypes.c_uint32), ("state", ctypes.c_int),
                ("control", ctypes.c_ubyte), ("needInitDic", ctypes.c_int),
                ("needInitState", ctypes.c_int), ("needInitProp", ctypes.c_int)]


class StreamDesc(ctypes.Structure):
    _fields_ = [("src_off", ctypes.c_uint64), ("src_len", ctypes.c_uint64),
                ("dst_off", ctypes.c_uint64), ("dst_cap", ctypes.c_uint64),
                ("probs_off", ctypes.c_uint64), ("props", ctypes.c_ubyte * 5),
                ("props_size", ctypes.c_ubyte), ("finish_mode", ctypes.c_ubyte),
                ("kind", ctypes.c_ubyte)]


class Result(ctypes.Structure):
    _fields_ = [("res", ctypes.c_int32), ("status", ctypes.c_int32),
                ("dest_len", ctypes.c_uint64), ("src_len", ctypes.c_uint64)]


class LdsClass(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("lanes_per_group", ctypes.c_uint32),
                ("lds_cells_per_lane", ctypes.c_uint32), ("groups_per_cu", ctypes.c_uint32),
                ("waves_per_simd", ctypes.c_uint32), ("lds_mask", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("slot_off", ctypes.c_uint64),
                ("slot_cells", ctypes.c_uint32), ("slot_groups", ctypes.c_uint32)]


class Plan(ctypes.Structure):
    _fields_ = [("workspace_bytes", ctypes.c_uint64), ("n", ctypes.c_uint64),
                ("n_lds", ctypes.c_uint64), ("lanes_per_group", ctypes.c_uint32),
                ("lds_cells_per_lane", ctypes.c_uint32), ("groups_per_cu", ctypes.c_uint32),
                ("waves_per_simd", ctypes.c_uint32), ("queue_offset", ctypes.c_uint64),
                ("persistent", ctypes.c_uint32), ("n_classes", ctypes.c_uint32),
                ("classes", LdsClass * 4)]


class PlanOptions(ctypes.Structure):
    """LzmaGpuPlanOptions (include/lzma_gpu.h): per-call planner overrides."""
    _fields_ = [("kernel", ctypes.c_uint32), ("cus", ctypes.c_uint32),
                ("lanes_per_group", ctypes.c_uint32), ("groups_per_cu", ctypes.c_uint32),
                ("waves_per_simd", ctypes.c_uint32), ("persistent", ctypes.c_uint32),
                ("coop", ctypes.c_uint32), ("one_class", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


KERNELS = {"auto": 0, "throughput": 1, "latency": 2, "coop": 3, "global": 4}


def plan_options(kernel="auto", **kw):
    """PlanOptions from a kernel name ('auto', 'throughput', 'latency', 'coop',
    'global') and any other LzmaGpuPlanOptions field by name."""
    o = PlanOptions()
    o.kernel = KERNELS[kernel]
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class SlicedPlan(ctypes.Structure):
    """LzmaGpuSlicedPlan (include/lzma_gpu.h): a time-sliced batch."""
    _fields_ = [("workspace_bytes", ctypes.c_uint64), ("n", ctypes.c_uint64),
                ("slice_bytes", ctypes.c_uint64), ("rounds", ctypes.c_uint32),
                ("kernel", ctypes.c_uint32), ("table_cells", ctypes.c_uint32),
                ("groups_per_cu", ctypes.c_uint32), ("max_groups", ctypes.c_uint32),
                ("lds_mask", ctypes.c_uint32), ("sess_off", ctypes.c_uint64),
                ("list_off", ctypes.c_uint64), ("ctr_off", ctypes.c_uint64),
                ("n_inplace", ctypes.c_uint64)]


SLICED_KERNELS = {"auto": 0, "lane": 1, "coop": 2, "global": 3}


class Session(ctypes.Structure):
    """LzmaGpuSession: a device-resident decoder (include/lzma_gpu.h)."""
    _fields_ = [("lc", ctypes.c_uint32), ("lp", ctypes.c_uint32), ("pb", ctypes.c_uint32),
                ("dict_size", ctypes.c_uint32), ("probs", ctypes.c_void_p),
                ("dic", ctypes.c_void_p), ("in_", ctypes.c_void_p),
                ("dic_buf_size", ctypes.c_uint64), ("dic_pos", ctypes.c_uint64),
                ("dic_limit", ctypes.c_uint64), ("in_len", ctypes.c_uint64),
                ("in_used", ctypes.c_uint64), ("range", ctypes.c_uint32),
                ("code", ctypes.c_uint32), ("processed_pos", ctypes.c_uint32),
                ("check_dic_size", ctypes.c_uint32), ("state", ctypes.c_uint32),
                ("reps", ctypes.c_uint32 * 4), ("remain_len", ctypes.c_uint32),
                ("need_flush", ctypes.c_uint32), ("need_init_state", ctypes.c_uint32),
                ("temp_buf_size", ctypes.c_uint32), ("finish_mode", ctypes.c_int32),
                ("res", ctypes.c_int32), ("status", ctypes.c_int32), ("mode", ctypes.c_int32),
                ("temp_buf", ctypes.c_ubyte * 20), ("_pad", ctypes.c_ubyte * 4),
                ("out", ctypes.c_void_p), ("out_len", ctypes.c_uint64)]


class XzBlock(ctypes.Structure):
    """LzmaGpuXzBlock (include/lzma_gpu.h): one block of an indexed xz file."""
    _fields_ = [("header_off", ctypes.c_uint64), ("data_off", ctypes.c_uint64),
                ("pack_size", ctypes.c_uint64), ("unpack_size", ctypes.c_uint64),
                ("dst_off", ctypes.c_uint64), ("check_off", ctypes.c_uint64),
                ("check_type", ctypes.c_uint32), ("check_size", ctypes.c_uint32),
                ("lzma2_prop", ctypes.c_uint32), ("x86", ctypes.c_uint32),
                ("x86_ip", ctypes.c_uint32), ("stream", ctypes.c_uint32),
                ("num_filters", ctypes.c_uint32), ("filter_id", ctypes.c_uint32 * 3),
                ("filter_prop", ctypes.c_uint32 * 3)]


class Bcj2Job(ctypes.Structure):
    """Bcj2GpuJob (include/lzma_gpu.h): one BCJ2 decode, device pointers."""
    _fields_ = [("buf0", ctypes.c_void_p), ("buf1", ctypes.c_void_p), ("buf2", ctypes.c_void_p),
                ("buf3", ctypes.c_void_p), ("size0", ctypes.c_uint64), ("size1", ctypes.c_uint64),
                ("size2", ctypes.c_uint64), ("size3", ctypes.c_uint64), ("out", ctypes.c_void_p),
                ("out_size", ctypes.c_uint64)]


class Bcj2EncRange(ctypes.Structure):
    """Bcj2GpuEncRange: one output range of a BCJ2 encode, in the destination."""
    _fields_ = [("off", ctypes.c_uint64), ("cap", ctypes.c_uint64)]


class Bcj2EncDesc(ctypes.Structure):
    """Bcj2GpuEncDesc: one stream of a BCJ2 encode batch; out = main, call, jump, rc."""
    _fields_ = [("src_off", ctypes.c_uint64), ("src_len", ctypes.c_uint64),
                ("out", Bcj2EncRange * 4)]


class Bcj2EncResult(ctypes.Structure):
    """Bcj2GpuEncResult: res and the four true lengths (main, call, jump, rc)."""
    _fields_ = [("res", ctypes.c_int32), ("_pad", ctypes.c_uint32), ("len", ctypes.c_uint64 * 4)]


class CSha256(ctypes.Structure):
    """CSha256 (Sha256.h:13-18): the drop-in hash state, the reference's layout."""
    _fields_ = [("state", ctypes.c_uint32 * 8), ("count", ctypes.c_uint64),
                ("buffer", ctypes.c_ubyte * 64)]


class Ppmd7StreamDesc(ctypes.Structure):
    """Ppmd7GpuStreamDesc (include/lzma_gpu.h): one PPMd7 stream of a batch."""
    _fields_ = [("src_off", ctypes.c_uint64), ("src_len", ctypes.c_uint64),
                ("dst_off", ctypes.c_uint64), ("dst_len", ctypes.c_uint64),
                ("ws_off", ctypes.c_uint64), ("mem_size", ctypes.c_uint32),
                ("order", ctypes.c_uint32)]


class Ppmd7Result(ctypes.Structure):
    """Ppmd7GpuResult: SzDecodePpmd's outcome for one stream."""
    _fields_ = [("res", ctypes.c_int32), ("_pad", ctypes.c_uint32), ("dest_len", ctypes.c_uint64),
                ("src_len", ctypes.c_uint64)]


class Ppmd7EncDesc(ctypes.Structure):
    """Ppmd7GpuEncDesc (include/lzma_gpu.h): one plain buffer of an encode batch."""
    _fields_ = [("src_off", ctypes.c_uint64), ("src_len", ctypes.c_uint64),
                ("dst_off", ctypes.c_uint64), ("dst_cap", ctypes.c_uint64),
                ("ws_off", ctypes.c_uint64), ("mem_size", ctypes.c_uint32),
                ("order", ctypes.c_uint32)]


class Ppmd7EncResult(ctypes.Structure):
    """Ppmd7GpuEncResult: res, bytes written, length of the whole stream."""
    _fields_ = [("res", ctypes.c_int32), ("_pad", ctypes.c_uint32), ("dest_len", ctypes.c_uint64),
                ("packed_len", ctypes.c_uint64)]


class CLzmaEncProps(ctypes.Structure):
    """CLzmaEncProps (LzmaEnc.h:15-31)."""
    _fields_ = [("level", ctypes.c_int), ("dictSize", ctypes.c_uint32), ("lc", ctypes.c_int),
                ("lp", ctypes.c_int), ("pb", ctypes.c_int), ("algo", ctypes.c_int),
                ("fb", ctypes.c_int), ("btMode", ctypes.c_int), ("numHashBytes", ctypes.c_int),
                ("mc", ctypes.c_uint32), ("writeEndMark", ctypes.c_uint),
                ("numThreads", ctypes.c_int)]


class CLzma2EncProps(ctypes.Structure):
    """CLzma2EncProps (Lzma2Enc.h:13-19)."""
    _fields_ = [("lzmaProps", CLzmaEncProps), ("blockSize", ctypes.c_size_t),
                ("numBlockThreads", ctypes.c_int), ("numTotalThreads", ctypes.c_int)]


SeqRead = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                           ctypes.POINTER(ctypes.c_size_t))
SeqWrite = ctypes.CFUNCTYPE(ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
ProgressFn = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64)


class ISeqInStream(ctypes.Structure):
    _fields_ = [("Read", SeqRead)]


class ISeqOutStream(ctypes.Structure):
    _fields_ = [("Write", SeqWrite)]


class ICompressProgress(ctypes.Structure):
    _fields_ = [("Progress", ProgressFn)]


class EncStreamDesc(ctypes.Structure):
    """LzmaEncGpuStreamDesc (include/lzma_gpu.h): one stream of an encode batch."""
    _fields_ = [("src_off", ctypes.c_uint64), ("src_len", ctypes.c_uint64),
                ("dst_off", ctypes.c_uint64), ("dst_cap", ctypes.c_uint64),
                ("ws_off", ctypes.c_uint64), ("dict_size", ctypes.c_uint32),
                ("lc", ctypes.c_uint32), ("lp", ctypes.c_uint32), ("pb", ctypes.c_uint32),
                ("fb", ctypes.c_uint32), ("mc", ctypes.c_uint32),
                ("write_end_mark", ctypes.c_uint32), ("mode", ctypes.c_uint32)]


class EncResult(ctypes.Structure):
    """LzmaEncGpuResult: LzmaEncode's outcome for one stream."""
    _fields_ = [("res", ctypes.c_int32), ("_pad", ctypes.c_uint32), ("dest_len", ctypes.c_uint64)]


class XzFilter(ctypes.Structure):
    """LzmaGpuXzFilter: one filter of an xz block's chain in front of LZMA2."""
    _fields_ = [("id", ctypes.c_uint32), ("prop", ctypes.c_uint32)]


class Lzma86StreamDesc(ctypes.Structure):
    """Lzma86GpuStreamDesc: one stream of an Lzma86 batch."""
    _fields_ = [("src_off", ctypes.c_uint64), ("src_len", ctypes.c_uint64),
                ("dst_off", ctypes.c_uint64), ("dst_cap", ctypes.c_uint64),
                ("level", ctypes.c_int32), ("dictSize", ctypes.c_uint32),
                ("filterMode", ctypes.c_int32), ("reserved", ctypes.c_uint32)]


class Lzma86Result(ctypes.Structure):
    """Lzma86GpuResult: Lzma86_Encode's / Lzma86_Decode's outcome for one stream."""
    _fields_ = [("res", ctypes.c_int32), ("filter", ctypes.c_uint32),
                ("dest_len", ctypes.c_uint64), ("src_len", ctypes.c_uint64)]


class Lzma86Stats(ctypes.Structure):
    """Lzma86GpuStats."""
    _fields_ = [("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("candidates", ctypes.c_uint64), ("filtered", ctypes.c_uint64),
                ("encode_launches", ctypes.c_uint64), ("stage_ns", ctypes.c_uint64 * 4)]


class EncSession(ctypes.Structure):
    """LzmaEncGpuSession (include/lzma_gpu.h, 200 bytes): a device-resident
    fast-mode encoder fed in pieces."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("ws", ctypes.c_void_p),
                ("src_cap", ctypes.c_uint64), ("dst_cap", ctypes.c_uint64),
                ("src_len", ctypes.c_uint64), ("in_budget", ctypes.c_uint64),
                ("in_pos", ctypes.c_uint64), ("out_pos", ctypes.c_uint64),
                ("dict_size", ctypes.c_uint32), ("lc", ctypes.c_uint32), ("lp", ctypes.c_uint32),
                ("pb", ctypes.c_uint32), ("fb", ctypes.c_uint32), ("mc", ctypes.c_uint32),
                ("write_end_mark", ctypes.c_uint32), ("finish", ctypes.c_uint32),
                ("res", ctypes.c_int32), ("status", ctypes.c_int32),
                ("needs_init", ctypes.c_uint32), ("finished", ctypes.c_uint32),
                ("overflow", ctypes.c_uint32), ("off", ctypes.c_uint32),
                ("cyclic_pos", ctypes.c_uint32), ("longest_match_length", ctypes.c_uint32),
                ("num_pairs", ctypes.c_uint32), ("num_avail", ctypes.c_uint32),
                ("additional_offset", ctypes.c_uint32), ("reps", ctypes.c_uint32 * 4),
                ("state", ctypes.c_uint32), ("range", ctypes.c_uint32), ("cache", ctypes.c_uint32),
                ("cache_size", ctypes.c_uint32), ("_pad", ctypes.c_uint32),
                ("low", ctypes.c_uint64), ("out_total", ctypes.c_uint64)]


class SzFolder(ctypes.Structure):
    """LzmaGpu7zFolder (include/lzma_gpu.h): one folder of an opened 7z archive."""
    _fields_ = [("pack_off", ctypes.c_uint64), ("pack_size", ctypes.c_uint64),
                ("unpack_size", ctypes.c_uint64), ("dst_off", ctypes.c_uint64),
                ("method", ctypes.c_uint64), ("x86", ctypes.c_uint32),
                ("supported", ctypes.c_uint32), ("crc_defined", ctypes.c_uint32),
                ("crc", ctypes.c_uint32), ("first_file", ctypes.c_uint32),
                ("num_files", ctypes.c_uint32), ("num_coders", ctypes.c_uint32),
                ("props_size", ctypes.c_uint32), ("props", ctypes.c_ubyte * 8)]


class SzFile(ctypes.Structure):
    """LzmaGpu7zFile (include/lzma_gpu.h): one file entry of an opened 7z archive."""
    _fields_ = [("size", ctypes.c_uint64), ("dst_off", ctypes.c_uint64),
                ("folder", ctypes.c_uint32), ("crc", ctypes.c_uint32),
                ("crc_defined", ctypes.c_uint32), ("has_stream", ctypes.c_uint32),
                ("is_dir", ctypes.c_uint32), ("name_off", ctypes.c_uint32),
                ("name_len", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]



class SzItem(ctypes.Structure):
    """LzmaGpu7zItem (include/lzma_gpu.h): one entry of an archive to write."""
    _fields_ = [("src_off", ctypes.c_uint64), ("size", ctypes.c_uint64),
                ("name_off", ctypes.c_uint32), ("name_len", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("method", ctypes.c_uint32)]


class SzMethod(ctypes.Structure):
    """LzmaGpu7zMethod: one row of the writer's method table."""
    _fields_ = [("method", ctypes.c_uint64), ("filter", ctypes.c_uint32),
                ("ppmd_order", ctypes.c_uint32), ("ppmd_mem_size", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("props", CLzma2EncProps)]


class SzWriteOptions(ctypes.Structure):
    _fields_ = [("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("workspace_limit", ctypes.c_uint64)]


class SzWriteStats(ctypes.Structure):
    _fields_ = [("folders", ctypes.c_uint64), ("pieces", ctypes.c_uint64),
                ("reencoded", ctypes.c_uint64), ("pack_bytes", ctypes.c_uint64),
                ("header_bytes", ctypes.c_uint64), ("encode_launches", ctypes.c_uint64),
                ("stage_ns", ctypes.c_uint64 * 8)]


class SzBcj2Info(ctypes.Structure):
    """LzmaGpu7zBcj2Info: what the header needs for one four-coder (BCJ2) folder."""
    _fields_ = [("pack_size", ctypes.c_uint64 * 4), ("unpack_size", ctypes.c_uint64 * 3),
                ("call_props", ctypes.c_ubyte * 5), ("jump_props", ctypes.c_ubyte * 5),
                ("reserved", ctypes.c_ubyte * 6)]


class SzPackPiece(ctypes.Structure):
    """SzGpuPackPiece: one piece of the pack stage's table."""
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint64), ("slot", ctypes.c_uint32),
                ("folder", ctypes.c_uint32), ("kind", ctypes.c_uint16), ("base", ctypes.c_uint16),
                ("flags", ctypes.c_uint32)]


class SzPackArgs(ctypes.Structure):
    """SzGpuPackArgs: device pointers as integers."""
    _fields_ = [("d_pieces", ctypes.c_void_p), ("n", ctypes.c_uint64),
                ("n_folders", ctypes.c_uint64), ("bases", ctypes.c_void_p * 4),
                ("d_lzma", ctypes.c_void_p), ("n_lzma", ctypes.c_uint64),
                ("d_lzma2", ctypes.c_void_p), ("n_lzma2", ctypes.c_uint64),
                ("d_ppmd", ctypes.c_void_p), ("n_ppmd", ctypes.c_uint64),
                ("d_out", ctypes.c_void_p), ("out_cap", ctypes.c_uint64),
                ("d_scratch", ctypes.c_void_p), ("d_piece_off", ctypes.c_void_p),
                ("d_folder_size", ctypes.c_void_p), ("d_total", ctypes.c_void_p)]


assert ctypes.sizeof(XzBlock) == 104 and ctypes.sizeof(Bcj2Job) == 80
assert ctypes.sizeof(Bcj2EncDesc) == 80 and ctypes.sizeof(Bcj2EncResult) == 40
assert ctypes.sizeof(SzFolder) == 80 and ctypes.sizeof(SzFile) == 48
assert ctypes.sizeof(StreamDesc) == 48 and ctypes.sizeof(Result) == 24
assert ctypes.sizeof(Session) == 192 and ctypes.sizeof(Plan) == 248
assert ctypes.sizeof(PlanOptions) == 40
assert ctypes.sizeof(CLzmaDec) == 136
assert ctypes.sizeof(CSha256) == 104
assert ctypes.sizeof(Ppmd7StreamDesc) == 48 and ctypes.sizeof(Ppmd7Result) == 24
assert ctypes.sizeof(Ppmd7EncDesc) == 48 and ctypes.sizeof(Ppmd7EncResult) == 24
assert ctypes.sizeof(CLzmaEncProps) == 48
assert ctypes.sizeof(EncStreamDesc) == 72 and ctypes.sizeof(EncResult) == 16
assert ctypes.sizeof(SzItem) == 32 and ctypes.sizeof(SzMethod) == 88
assert ctypes.sizeof(SzWriteOptions) == 16 and ctypes.sizeof(SzWriteStats) == 112
assert ctypes.sizeof(SzBcj2Info) == 72
assert ctypes.sizeof(SzPackPiece) == 32 and ctypes.sizeof(SzPackArgs) == 152

_P = ctypes.c_void_p
_sig = {
    "LzmaProps_Decode": (ctypes.c_int, [ctypes.POINTER(CLzmaProps), ctypes.c_char_p, ctypes.c_uint]),
    "LzmaDec_AllocateProbs": (ctypes.c_int, [ctypes.POINTER(CLzmaDec), ctypes.c_char_p, ctypes.c_uint, ctypes.POINTER(ISzAlloc)]),
    "LzmaDec_FreeProbs": (None, [ctypes.POINTER(CLzmaDec), ctypes.POINTER(ISzAlloc)]),
    "LzmaDec_Allocate": (ctypes.c_int, [ctypes.POINTER(CLzmaDec), ctypes.c_char_p, ctypes.c_uint, ctypes.POINTER(ISzAlloc)]),
    "LzmaDec_Free": (None, [ctypes.POINTER(CLzmaDec), ctypes.POINTER(ISzAlloc)]),
    "LzmaDec_Init": (None, [ctypes.POINTER(CLzmaDec)]),
    "LzmaDec_InitDicAndState": (None, [ctypes.POINTER(CLzmaDec), ctypes.c_int, ctypes.c_int]),
    "LzmaDec_DecodeToDic": (ctypes.c_int, [ctypes.POINTER(CLzmaDec), ctypes.c_size_t, _P, _sp, ctypes.c_int, _ip]),
    "LzmaDec_DecodeToBuf": (ctypes.c_int, [ctypes.POINTER(CLzmaDec), _P, _sp, _P, _sp, ctypes.c_int, _ip]),
    "LzmaGpu_DecoderRelease": (None, [ctypes.POINTER(CLzmaDec)]),
    "LzmaGpu_DropinTransferStats": (None, [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
    "LzmaGpu_CoalesceStats": (None, [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
    "LzmaGpu_DropinPathStats": (None, [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
    "LzmaDecode": (ctypes.c_int, [_P, _sp, _P, _sp, ctypes.c_char_p, ctypes.c_uint, ctypes.c_int, _ip, ctypes.POINTER(ISzAlloc)]),
    "LzmaUncompress": (ctypes.c_int, [_P, _sp, _P, _sp, ctypes.c_char_p, ctypes.c_size_t]),
    "Lzma2Dec_AllocateProbs": (ctypes.c_int, [ctypes.POINTER(CLzma2Dec), ctypes.c_ubyte, ctypes.POINTER(ISzAlloc)]),
    "Lzma2Dec_Allocate": (ctypes.c_int, [ctypes.POINTER(CLzma2Dec), ctypes.c_ubyte, ctypes.POINTER(ISzAlloc)]),
    "Lzma2Dec_Init": (None, [ctypes.POINTER(CLzma2Dec)]),
    "Lzma2Dec_DecodeToDic": (ctypes.c_int, [ctypes.POINTER(CLzma2Dec), ctypes.c_size_t, _P, _sp, ctypes.c_int, _ip]),
    "Lzma2Dec_DecodeToBuf": (ctypes.c_int, [ctypes.POINTER(CLzma2Dec), _P, _sp, _P, _sp, ctypes.c_int, _ip]),
    "Lzma2Decode": (ctypes.c_int, [_P, _sp, _P, _sp, ctypes.c_ubyte, ctypes.c_int, _ip, ctypes.POINTER(ISzAlloc)]),
    "LzmaGpu_PlanBatch": (ctypes.c_size_t, [ctypes.POINTER(StreamDesc), ctypes.c_size_t, _P]),
    "LzmaGpu_DecodeBatch": (ctypes.c_int, [_P, _P, ctypes.c_size_t, _P, _P, _P, ctypes.c_size_t, _P, _P]),
    "LzmaGpu_PlanBatchEx": (ctypes.c_int, [ctypes.POINTER(StreamDesc), ctypes.c_size_t, _P, ctypes.POINTER(Plan)]),
    "LzmaGpu_DecodeBatchEx": (ctypes.c_int, [ctypes.POINTER(Plan), _P, _P, _P, _P, _P, _P, _P]),
    "LzmaGpu_DecodeBatchHost": (ctypes.c_int, [ctypes.POINTER(StreamDesc), ctypes.c_size_t, _P, ctypes.c_size_t, _P, ctypes.c_size_t, ctypes.POINTER(Result)]),
    "LzmaGpu_PlanBatchOpt": (ctypes.c_int, [ctypes.POINTER(StreamDesc), ctypes.c_size_t, _P, ctypes.POINTER(Plan), ctypes.POINTER(PlanOptions)]),
    "LzmaGpu_DecodeBatchHostOpt": (ctypes.c_int, [ctypes.POINTER(StreamDesc), ctypes.c_size_t, _P, ctypes.c_size_t, _P, ctypes.c_size_t, ctypes.POINTER(Result), ctypes.POINTER(PlanOptions), ctypes.POINTER(Plan)]),
    "Lzma2Gpu_SplitBlocks": (ctypes.c_size_t, [_P, ctypes.c_size_t, _P, _P, _P, ctypes.c_size_t]),
    "LzmaGpu_SessionProbsBytes": (ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_uint]),
    "LzmaGpu_SessionInit": (ctypes.c_int, [ctypes.POINTER(Session), ctypes.c_char_p, ctypes.c_uint, _P, _P, ctypes.c_size_t]),
    "LzmaGpu_SessionDecodeBatch": (ctypes.c_int, [_P, ctypes.c_size_t, _P]),
    "LzmaGpu_PlanSliced": (ctypes.c_int, [ctypes.POINTER(StreamDesc), ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint, _P, ctypes.POINTER(SlicedPlan)]),
    "LzmaGpu_DecodeBatchSliced": (ctypes.c_int, [ctypes.POINTER(SlicedPlan), _P, _P, _P, _P, _P, _P, ctypes.c_uint, ctypes.c_uint, _P]),
    "LzmaGpu_SlicedActive": (ctypes.c_int, [ctypes.POINTER(SlicedPlan), _P, ctypes.c_uint, _sp, _P]),
    "LzmaGpu_DecodeBatchSlicedHost": (ctypes.c_int, [ctypes.POINTER(StreamDesc), ctypes.c_size_t, _P, ctypes.c_size_t, _P, ctypes.c_size_t, ctypes.POINTER(Result), ctypes.c_uint64, ctypes.c_uint, ctypes.POINTER(SlicedPlan)]),
    "CrcGenerateTable": (None, []),
    "CrcUpdate": (ctypes.c_uint32, [ctypes.c_uint32, _P, ctypes.c_size_t]),
    "CrcCalc": (ctypes.c_uint32, [_P, ctypes.c_size_t]),
    "CrcGpu_PlanChunks": (ctypes.c_size_t, [_P, ctypes.c_size_t, _P, _P]),
    "CrcGpu_Batch": (ctypes.c_int, [_P, _P, _P, ctypes.c_size_t, _P, _P, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, _P, _P, _P]),
    "LzmaGpu_Crc32Plan": (ctypes.c_size_t, [ctypes.POINTER(StreamDesc), ctypes.c_size_t, _P, _P]),
    "LzmaGpu_Crc32Batch": (ctypes.c_int, [_P, _P, ctypes.c_size_t, _P, _P, _P, ctypes.c_size_t, _P, _P, _P]),
    "x86_Convert": (ctypes.c_size_t, [_P, ctypes.c_size_t, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int]),
    "BcjGpu_X86Batch": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, ctypes.c_size_t, ctypes.c_int, _P]),
    "ARM_Convert": (ctypes.c_size_t, [_P, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int]),
    "ARMT_Convert": (ctypes.c_size_t, [_P, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int]),
    "PPC_Convert": (ctypes.c_size_t, [_P, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int]),
    "SPARC_Convert": (ctypes.c_size_t, [_P, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int]),
    "IA64_Convert": (ctypes.c_size_t, [_P, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int]),
    "Delta_Init": (None, [_P]),
    "Delta_Encode": (None, [_P, ctypes.c_uint, _P, ctypes.c_size_t]),
    "Delta_Decode": (None, [_P, ctypes.c_uint, _P, ctypes.c_size_t]),
    "BraGpu_Batch": (ctypes.c_int, [ctypes.c_uint, _P, _P, _P, _P, _P, ctypes.c_size_t, ctypes.c_int, _P]),
    "DeltaGpu_Batch": (ctypes.c_int, [_P, _P, _P, _P, _P, ctypes.c_size_t, ctypes.c_int, _P]),
    "Bcj2_Decode": (ctypes.c_int, [_P, ctypes.c_size_t, _P, ctypes.c_size_t, _P, ctypes.c_size_t, _P, ctypes.c_size_t, _P, ctypes.c_size_t]),
    "Bcj2Gpu_Batch": (ctypes.c_int, [_P, ctypes.c_size_t, _P, _P]),
    "Bcj2EncGpu_Bound": (None, [ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    "Bcj2EncGpu_Scratch": (ctypes.c_uint64, [ctypes.POINTER(Bcj2EncDesc), ctypes.c_size_t]),
    "Bcj2EncGpu_EncodeBatch": (ctypes.c_int, [_P, ctypes.c_size_t, _P, _P, _P, _P, _P]),
    "Bcj2EncGpu_EncodeBatchHost": (ctypes.c_int, [ctypes.POINTER(Bcj2EncDesc), ctypes.c_size_t, _P,
                                                  ctypes.c_size_t, _P, ctypes.c_size_t,
                                                  ctypes.POINTER(Bcj2EncResult), ctypes.c_uint64]),
    "Crc64Calc": (ctypes.c_uint64, [_P, ctypes.c_size_t]),
    "Crc64Gpu_Batch": (ctypes.c_int, [_P, _P, _P, ctypes.c_size_t, _P, _P, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64, _P, _P, _P]),
    "Sha256_Init": (None, [ctypes.POINTER(CSha256)]),
    "Sha256_Update": (None, [ctypes.POINTER(CSha256), _P, ctypes.c_size_t]),
    "Sha256_Final": (None, [ctypes.POINTER(CSha256), _P]),
    "Sha256Gpu_Batch": (ctypes.c_int, [_P, _P, _P, ctypes.c_size_t, ctypes.c_uint, _P, _P]),
    "LzmaGpu_XzIndex": (ctypes.c_int, [_P, ctypes.c_size_t, ctypes.POINTER(XzBlock), ctypes.c_size_t, _sp, ctypes.POINTER(ctypes.c_uint64)]),
    "LzmaGpu_XzDecode": (ctypes.c_int, [_P, _sp, _P, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int64)]),
    "LzmaGpu_7zOpen": (ctypes.c_int, [_P, ctypes.c_size_t, _P, ctypes.c_size_t, _sp, _P,
                                      ctypes.c_size_t, _sp, _P, ctypes.c_size_t, _sp,
                                      ctypes.POINTER(ctypes.c_uint64)]),
    "LzmaGpu_7zExtract": (ctypes.c_int, [_P, _sp, _P, ctypes.c_size_t, _P, ctypes.c_size_t]),
    "LzmaGpu_7zOpenEx": (ctypes.c_int, [_P, ctypes.c_size_t, _P, ctypes.c_size_t, _sp, _P,
                                        ctypes.c_size_t, _sp, _P, ctypes.c_size_t, _sp,
                                        ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint]),
    "LzmaGpu_7zExtractEx": (ctypes.c_int, [_P, _sp, _P, ctypes.c_size_t, _P, ctypes.c_size_t,
                                           ctypes.c_uint]),
    "Ppmd7Gpu_WorkspaceBytes": (ctypes.c_uint64, [ctypes.c_uint32]),
    "Ppmd7Gpu_DecodeBatch": (ctypes.c_int, [_P, ctypes.c_size_t, _P, _P, _P, _P, _P]),
    "Ppmd7Gpu_DecodeBatchHost": (ctypes.c_int, [ctypes.POINTER(Ppmd7StreamDesc), ctypes.c_size_t, _P,
                                                ctypes.c_size_t, _P, ctypes.c_size_t,
                                                ctypes.POINTER(Ppmd7Result), ctypes.c_uint64]),
    "Ppmd7Gpu_EncodeBatch": (ctypes.c_int, [_P, ctypes.c_size_t, _P, _P, _P, _P, _P]),
    "Ppmd7Gpu_EncodeBatchHost": (ctypes.c_int, [ctypes.POINTER(Ppmd7EncDesc), ctypes.c_size_t, _P,
                                                ctypes.c_size_t, _P, ctypes.c_size_t,
                                                ctypes.POINTER(Ppmd7EncResult), ctypes.c_uint64]),
    "LzmaEncProps_Init": (None, [ctypes.POINTER(CLzmaEncProps)]),
    "LzmaEncProps_Normalize": (None, [ctypes.POINTER(CLzmaEncProps)]),
    "LzmaEncProps_GetDictSize": (ctypes.c_uint32, [ctypes.POINTER(CLzmaEncProps)]),
    "LzmaEncGpu_DescFromProps": (ctypes.c_int, [ctypes.POINTER(CLzmaEncProps), ctypes.c_int,
                                                ctypes.POINTER(EncStreamDesc), ctypes.c_char_p]),
    "LzmaEncGpu_DescFromPropsEx": (ctypes.c_int, [ctypes.POINTER(CLzmaEncProps), ctypes.c_int,
                                                  ctypes.c_uint, ctypes.POINTER(EncStreamDesc),
                                                  ctypes.c_char_p]),
    "LzmaEncGpu_SetModes": (ctypes.c_uint, [ctypes.c_uint]),
    "LzmaEncGpu_GetModes": (ctypes.c_uint, []),
    "Lzma2EncGpu_DescFromPropsEx": (ctypes.c_int, [ctypes.POINTER(CLzma2EncProps), ctypes.c_uint,
                                                   ctypes.POINTER(EncStreamDesc),
                                                   ctypes.POINTER(ctypes.c_ubyte)]),
    "LzmaEncGpu_PlanBatch": (ctypes.c_int, [ctypes.POINTER(EncStreamDesc), ctypes.c_size_t, _P,
                                            ctypes.POINTER(ctypes.c_uint64)]),
    "LzmaEncGpu_EncodeBatch": (ctypes.c_int, [_P, _P, ctypes.c_size_t, _P, _P, _P, _P,
                                              ctypes.c_uint, _P]),
    "LzmaEncGpu_EncodeBatchHost": (ctypes.c_int, [ctypes.POINTER(EncStreamDesc), ctypes.c_size_t,
                                                  _P, ctypes.c_size_t, _P, ctypes.c_size_t,
                                                  ctypes.POINTER(EncResult), ctypes.c_uint64]),
    "LzmaEncode": (ctypes.c_int, [_P, _sp, _P, ctypes.c_size_t, ctypes.POINTER(CLzmaEncProps), _P,
                                  _sp, ctypes.c_int, _P, _P, _P]),
    "LzmaCompress": (ctypes.c_int, [_P, _sp, _P, ctypes.c_size_t, _P, _sp, ctypes.c_int,
                                    ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, ctypes.c_int]),
    "Lzma2EncProps_Init": (None, [ctypes.POINTER(CLzma2EncProps)]),
    "Lzma2EncProps_Normalize": (None, [ctypes.POINTER(CLzma2EncProps)]),
    "Lzma2EncGpu_BlockBound": (ctypes.c_size_t, [ctypes.c_size_t]),
    "Lzma2EncGpu_DescFromProps": (ctypes.c_int, [ctypes.POINTER(CLzma2EncProps),
                                                 ctypes.POINTER(EncStreamDesc),
                                                 ctypes.POINTER(ctypes.c_ubyte)]),
    "Lzma2EncGpu_PlanBatch": (ctypes.c_int, [ctypes.POINTER(EncStreamDesc), ctypes.c_size_t, _P,
                                             ctypes.POINTER(ctypes.c_uint64)]),
    "Lzma2EncGpu_EncodeBatch": (ctypes.c_int, [_P, _P, ctypes.c_size_t, _P, _P, _P, _P,
                                               ctypes.c_uint, _P]),
    "Lzma2EncGpu_EncodeBatchHost": (ctypes.c_int, [ctypes.POINTER(EncStreamDesc), ctypes.c_size_t,
                                                   _P, ctypes.c_size_t, _P, ctypes.c_size_t,
                                                   ctypes.POINTER(EncResult), ctypes.c_uint64]),
    "Lzma2EncGpu_Compact": (ctypes.c_int, [_P, _P, ctypes.c_size_t, _P, _P, ctypes.c_uint64, _P, _P,
                                           _P]),
    "LzmaGpu_Lzma2EncodeHost": (ctypes.c_int, [_P, _sp, _P, ctypes.c_size_t,
                                               ctypes.POINTER(CLzma2EncProps),
                                               ctypes.POINTER(ctypes.c_ubyte)]),
    "LzmaEncGpu_SessionWorkspaceBytes": (ctypes.c_uint64, [ctypes.POINTER(CLzmaEncProps),
                                                           ctypes.c_uint64]),
    "LzmaEncGpu_SessionInit": (ctypes.c_int, [ctypes.POINTER(EncSession),
                                              ctypes.POINTER(CLzmaEncProps), ctypes.c_int, _P,
                                              ctypes.c_uint64, _P, ctypes.c_uint64, _P, _P]),
    "LzmaEncGpu_SessionScratchBytes": (ctypes.c_size_t, [ctypes.c_size_t]),
    "LzmaEncGpu_SessionEncodeBatch": (ctypes.c_int, [_P, ctypes.c_size_t, _P, ctypes.c_uint, _P]),
    "LzmaEncGpu_SessionListPass": (ctypes.c_int, [_P, ctypes.c_size_t, _P, _P]),
    "LzmaEnc_Create": (ctypes.c_void_p, [ctypes.POINTER(ISzAlloc)]),
    "LzmaEnc_Destroy": (None, [ctypes.c_void_p, ctypes.POINTER(ISzAlloc),
                               ctypes.POINTER(ISzAlloc)]),
    "LzmaEnc_SetProps": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(CLzmaEncProps)]),
    "LzmaEnc_WriteProperties": (ctypes.c_int, [ctypes.c_void_p, _P, _sp]),
    "LzmaEnc_Encode": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ISeqOutStream),
                                      ctypes.POINTER(ISeqInStream),
                                      ctypes.POINTER(ICompressProgress), _P, _P]),
    "LzmaEnc_MemEncode": (ctypes.c_int, [ctypes.c_void_p, _P, _sp, _P, ctypes.c_size_t,
                                         ctypes.c_int, _P, _P, _P]),
    "Lzma2Enc_Create": (ctypes.c_void_p, [ctypes.POINTER(ISzAlloc), ctypes.POINTER(ISzAlloc)]),
    "Lzma2Enc_Destroy": (None, [ctypes.c_void_p]),
    "Lzma2Enc_SetProps": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(CLzma2EncProps)]),
    "Lzma2Enc_WriteProperties": (ctypes.c_ubyte, [ctypes.c_void_p]),
    "Lzma2Enc_Encode": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ISeqOutStream),
                                       ctypes.POINTER(ISeqInStream), _P]),
    "LzmaGpu_XzEncode": (ctypes.c_int, [_P, _sp, _P, ctypes.c_size_t,
                                        ctypes.POINTER(CLzma2EncProps), ctypes.c_uint]),
    "LzmaGpu_XzEncodeEx": (ctypes.c_int, [_P, _sp, _P, ctypes.c_size_t,
                                          ctypes.POINTER(CLzma2EncProps), ctypes.c_uint,
                                          ctypes.POINTER(XzFilter), ctypes.c_uint]),
    "Lzma86Gpu_EncodeScratch": (ctypes.c_int, [ctypes.POINTER(Lzma86StreamDesc), ctypes.c_size_t,
                                               ctypes.POINTER(ctypes.c_uint64)]),
    "Lzma86Gpu_EncodeBatch": (ctypes.c_int, [ctypes.POINTER(Lzma86StreamDesc), ctypes.c_size_t, _P,
                                             _P, _P, ctypes.c_uint64, _P, _P]),
    "Lzma86Gpu_EncodeBatchHost": (ctypes.c_int, [ctypes.POINTER(Lzma86StreamDesc), ctypes.c_size_t,
                                                 _P, ctypes.c_size_t, _P, ctypes.c_size_t,
                                                 ctypes.POINTER(Lzma86Result), ctypes.c_uint64,
                                                 ctypes.POINTER(Lzma86Stats)]),
    "Lzma86Gpu_DecodeScratch": (ctypes.c_int, [ctypes.POINTER(Lzma86StreamDesc), ctypes.c_size_t,
                                               _P, ctypes.POINTER(ctypes.c_uint64)]),
    "Lzma86Gpu_DecodeBatch": (ctypes.c_int, [ctypes.POINTER(Lzma86StreamDesc), ctypes.c_size_t, _P,
                                             _P, _P, _P, ctypes.c_uint64, _P, _P]),
    "Lzma86Gpu_DecodeBatchHost": (ctypes.c_int, [ctypes.POINTER(Lzma86StreamDesc), ctypes.c_size_t,
                                                 _P, ctypes.c_size_t, _P, ctypes.c_size_t,
                                                 ctypes.POINTER(Lzma86Result)]),
    "Lzma86_Encode": (ctypes.c_int, [_P, _sp, _P, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32,
                                     ctypes.c_int]),
    "Lzma86_GetUnpackSize": (ctypes.c_int, [_P, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]),
    "Lzma86_Decode": (ctypes.c_int, [_P, _sp, _P, _sp]),
    "LzmaGpu_7zWritePlan": (ctypes.c_int, [_P, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, _P,
                                           ctypes.c_size_t, _P, ctypes.c_size_t, _sp, _sp,
                                           ctypes.POINTER(ctypes.c_uint64)]),
    "LzmaGpu_7zWriteHeader": (ctypes.c_int, [_P, ctypes.c_size_t, _P, ctypes.c_size_t, _P, _P,
                                             ctypes.c_size_t, ctypes.c_uint, _P, ctypes.c_size_t,
                                             _sp, _P, ctypes.c_uint64]),
    "LzmaGpu_7zWriteHeaderEx": (ctypes.c_int, [_P, ctypes.c_size_t, _P, ctypes.c_size_t, _P, _P,
                                               ctypes.c_size_t, ctypes.c_uint, _P, ctypes.c_size_t,
                                               _P, ctypes.c_size_t, _sp, _P, ctypes.c_uint64]),
    "LzmaGpu_7zWrite": (ctypes.c_int, [_P, _sp, _P, ctypes.c_size_t, _P, ctypes.c_size_t, _P,
                                       ctypes.c_size_t, _P, ctypes.c_size_t,
                                       ctypes.POINTER(SzWriteOptions),
                                       ctypes.POINTER(SzWriteStats)]),
    "SzGpu_PackScratch": (ctypes.c_size_t, [ctypes.c_size_t]),
    "SzGpu_PackBatch": (ctypes.c_int, [ctypes.POINTER(SzPackArgs), _P]),
    "LzmaGpu_DeviceCount": (ctypes.c_int, []),
    "LzmaGpu_LastError": (ctypes.c_char_p, []),
    "LzmaGpu_Version": (ctypes.c_char_p, []),
}
for _name, (_rt, _at) in _sig.items():
    _f = getattr(_lib, _name)
    _f.restype = _rt
    _f.argtypes = _at

EXPORTED = tuple(_sig)
lib = _lib

_libc = ctypes.CDLL(None)
_libc.malloc.restype = ctypes.c_void_p
_libc.malloc.argtypes = [ctypes.c_size_t]
_libc.free.argtypes = [ctypes.c_void_p]


@ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
def _py_alloc(_p, n):
    return _libc.malloc(n if n else 1)


@ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p)
def _py_free(_p, a):
    _libc.free(a)


g_alloc = ISzAlloc(_py_alloc, _py_free)


def transfer_stats(reset=False):
    """(h2d_bytes, d2h_bytes, calls) of the drop-in entry points
    (LzmaGpu_DropinTransferStats); reset zeroes the counters after reading."""
    h, d, c = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.LzmaGpu_DropinTransferStats(ctypes.byref(h), ctypes.byref(d), ctypes.byref(c),
                                     1 if reset else 0)
    return h.value, d.value, c.value


DROPIN_PATHS = ("one_pinned", "one_pageable", "one_percall_out", "sess_pinned", "sess_unpinned",
                "sess_coop", "sess_global", "sess_mixed", "history_upload", "span_one",
                "span_two", "mirror_evicted", "pool_reused")


def path_stats(reset=False):
    """{path: count} of the drop-in decode entry points (LzmaGpu_DropinPathStats,
    LZMA_GPU_DROPIN_PATHS values); reset zeroes the counters after reading."""
    v = (ctypes.c_uint64 * len(DROPIN_PATHS))()
    _lib.LzmaGpu_DropinPathStats(v, 1 if reset else 0)
    return dict(zip(DROPIN_PATHS, v))


def last_error():
    return _lib.LzmaGpu_LastError().decode()


def device_count():
    return _lib.LzmaGpu_DeviceCount()


def _buf(data):
    return ctypes.create_string_buffer(bytes(data), max(len(data), 1))


# ---------------------------------------------------------------- one-call API

def coalesce_stats(reset=False):
    """(batches, calls, largest batch) of the one-call coalescer
    (LzmaGpu_CoalesceStats); reset zeroes the counters after reading."""
    b, c, m = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    _lib.LzmaGpu_CoalesceStats(ctypes.byref(b), ctypes.byref(c), ctypes.byref(m),
                               1 if reset else 0)
    return b.value, c.value, m.value


def LzmaDecode(src, props, dest_cap, finish=LZMA_FINISH_END):
    """LzmaDecode (LzmaDec.c:972). Returns (res, status, destLen, srcLen, out)."""
    s = _buf(src)
    d = ctypes.create_string_buffer(max(dest_cap, 1))
    dl = ctypes.c_size_t(dest_cap)
    sl = ctypes.c_size_t(len(src))
    st = ctypes.c_int(-1)
    res = _lib.LzmaDecode(d, ctypes.byref(dl), s, ctypes.byref(sl), bytes(props), len(props),
                          finish, ctypes.byref(st), ctypes.byref(g_alloc))
    return res, st.value, dl.value, sl.value, d.raw[:dl.value]


def LzmaUncompress(src, props, dest_cap):
    """LzmaUncompress (LzmaLib.c:41). Returns (res, destLen, srcLen, out)."""
    s = _buf(src)
    d = ctypes.create_string_buffer(max(dest_cap, 1))
    dl = ctypes.c_size_t(dest_cap)
    sl = ctypes.c_size_t(len(src))
    res = _lib.LzmaUncompress(d, ctypes.byref(dl), s, ctypes.byref(sl), bytes(props), len(props))
    return res, dl.value, sl.value, d.raw[:dl.value]


def Lzma2Decode(src, prop, dest_cap, finish=LZMA_FINISH_END):
    s = _buf(src)
    d = ctypes.create_string_buffer(max(dest_cap, 1))
    dl = ctypes.c_size_t(dest_cap)
    sl = ctypes.c_size_t(len(src))
    st = ctypes.c_int(-1)
    res = _lib.Lzma2Decode(d, ctypes.byref(dl), s, ctypes.byref(sl), prop, finish,
                           ctypes.byref(st), ctypes.byref(g_alloc))
    return res, st.value, dl.value, sl.value, d.raw[:dl.value]


# ---------------------------------------------------------------- streaming API

def stream_decode(src, props, out_total, in_chunk, out_chunk, finish, max_calls=100000):
    """zlib-like loop over LzmaDec_DecodeToBuf with bounded chunks -- the same
    contract as the oracle's orc_lzma_stream_decode / the fork's
    SzDecodeLzmaToFileWithBuf (7zDec.c:567-648).
    Returns (calls, trace[(res, status, srcLen, destLen)], out, in_used)."""
    dec = CLzmaDec()
    dec.dic = None
    dec.probs = None
    r = _lib.LzmaDec_Allocate(ctypes.byref(dec), bytes(props), 5, ctypes.byref(g_alloc))
    if r != SZ_OK:
        return -r, [], b"", 0
    _lib.LzmaDec_Init(ctypes.byref(dec))
    sbuf = _buf(src)
    out = ctypes.create_string_buffer(max(out_total, 1))
    base_s = ctypes.addressof(sbuf)
    base_o = ctypes.addressof(out)
    in_pos = out_pos = 0
    trace = []
    try:
        while len(trace) < max_calls:
            sl = ctypes.c_size_t(min(len(src) - in_pos, in_chunk))
            dl = ctypes.c_size_t(min(out_total - out_pos, out_chunk))
            st = ctypes.c_int(-1)
            res = _lib.LzmaDec_DecodeToBuf(ctypes.byref(dec), base_o + out_pos, ctypes.byref(dl),
                                           base_s + in_pos, ctypes.byref(sl), finish,
                                           ctypes.byref(st))
            trace.append((res, st.value, sl.value, dl.value))
            in_pos += sl.value
            out_pos += dl.value
            if res != SZ_OK or st.value == 1 or out_pos == out_total:
                break
            if sl.value == 0 and dl.value == 0:
                break
    finally:
        _lib.LzmaDec_Free(ctypes.byref(dec), ctypes.byref(g_alloc))
    return len(trace), trace, out.raw[:out_pos], in_pos


def dic_decode(src, props, out_total, win, max_calls=100000, out=None, between=None):
    """The 7zDec.c:127-171 (SzDecodeLzma) loop over LzmaDec_DecodeToDic:
    LzmaDec_AllocateProbs, dic = the whole output buffer (dicBufSize =
    out_total), LzmaDec_Init, then DecodeToDic(out_total, FINISH_END) over look
    windows of at most `win` input bytes -- the same contract as the oracle's
    orc_lzma_dic_decode.  `out` (optional): a ctypes buffer of >= out_total bytes
    to decode into.  `between` (optional): called with (call index, the
    CLzmaDec) after every call.  Returns (calls, trace[(res, status, srcLen,
    dicPos)], out bytes, in_used)."""
    dec = CLzmaDec()
    dec.dic = None
    dec.probs = None
    r = _lib.LzmaDec_AllocateProbs(ctypes.byref(dec), bytes(props), 5, ctypes.byref(g_alloc))
    if r != SZ_OK:
        return -r, [], b"", 0
    sbuf = _buf(src)
    if out is None:
        out = ctypes.create_string_buffer(max(out_total, 1))
    dec.dic = ctypes.addressof(out)
    dec.dicBufSize = out_total
    _lib.LzmaDec_Init(ctypes.byref(dec))
    base_s = ctypes.addressof(sbuf)
    in_pos = 0
    trace = []
    try:
        while len(trace) < max_calls:
            sl = ctypes.c_size_t(min(len(src) - in_pos, win))
            pos0 = dec.dicPos
            st = ctypes.c_int(-1)
            res = _lib.LzmaDec_DecodeToDic(ctypes.byref(dec), out_total, base_s + in_pos,
                                           ctypes.byref(sl), LZMA_FINISH_END, ctypes.byref(st))
            trace.append((res, st.value, sl.value, dec.dicPos))
            in_pos += sl.value
            if res != SZ_OK:
                break
            if dec.dicPos == out_total or (sl.value == 0 and dec.dicPos == pos0):
                break
            if between is not None:
                between(len(trace) - 1, dec)
    finally:
        _lib.LzmaDec_FreeProbs(ctypes.byref(dec), ctypes.byref(g_alloc))
    return len(trace), trace, out.raw[:dec.dicPos], in_pos


# ---------------------------------------------------------------- batch API

def make_descs(items):
    """items: list of dicts with src_off, src_len, dst_off, dst_cap, props(bytes),
    finish, kind.  Returns a ctypes StreamDesc array."""
    arr = (StreamDesc * len(items))()
    for i, it in enumerate(items):
        d = arr[i]
        d.src_off, d.src_len = it["src_off"], it["src_len"]
        d.dst_off, d.dst_cap = it["dst_off"], it["dst_cap"]
        p = bytes(it["props"])
        for k in range(min(len(p), 5)):
            d.props[k] = p[k]
        d.props_size = it.get("props_size", len(p))
        d.finish_mode = it.get("finish", LZMA_FINISH_END)
        d.kind = it.get("kind", KIND_LZMA)
    return arr


def decode_batch_host(descs, src, dst_bytes, opts=None, plan_out=None):
    """Decode a batch from host buffers.  Returns (res, results[ctypes], dst bytes).
    opts: PlanOptions (None = the planner's defaults); plan_out: a Plan to receive
    the plan that ran."""
    n = len(descs)
    res = (Result * max(n, 1))()
    s = _buf(src)
    d = ctypes.create_string_buffer(max(dst_bytes, 1))
    if opts is None and plan_out is None:
        r = _lib.LzmaGpu_DecodeBatchHost(descs, n, s, len(src), d, dst_bytes, res)
    else:
        r = _lib.LzmaGpu_DecodeBatchHostOpt(descs, n, s, len(src), d, dst_bytes, res,
                                            ctypes.byref(opts) if opts is not None else None,
                                            ctypes.byref(plan_out) if plan_out is not None
                                            else None)
    return r, res, d.raw[:dst_bytes]


def plan(descs, order=None):
    """Fill probs_off (and the lane order, a ctypes uint32 array). Returns workspace bytes."""
    return _lib.LzmaGpu_PlanBatch(descs, len(descs), order)


def plan_ex(descs, opts=None):
    """LzmaGpu_PlanBatchEx (or LzmaGpu_PlanBatchOpt when opts is a PlanOptions):
    returns (Plan, order[ctypes uint32 array])."""
    n = len(descs)
    order = (ctypes.c_uint32 * max(n, 1))()
    p = Plan()
    if opts is None:
        r = _lib.LzmaGpu_PlanBatchEx(descs, n, order, ctypes.byref(p))
    else:
        r = _lib.LzmaGpu_PlanBatchOpt(descs, n, order, ctypes.byref(p), ctypes.byref(opts))
    if r != SZ_OK:
        raise RuntimeError(f"LzmaGpu_PlanBatchEx failed: {r}")
    return p, order


def decode_batch_device_ex(plan, d_descs, d_order, d_src, d_dst, d_ws, d_results, stream=0):
    """LzmaGpu_DecodeBatchEx over raw device pointers (ints)."""
    return _lib.LzmaGpu_DecodeBatchEx(ctypes.byref(plan), d_descs, d_order, d_src, d_dst, d_ws,
                                      d_results, stream or None)


def decode_batch_device(d_descs, d_order, n, d_src, d_dst, d_ws, ws_bytes, d_results, stream=0):
    """All arguments are raw device pointers (ints); stream is a hipStream_t (int)."""
    return _lib.LzmaGpu_DecodeBatch(d_descs, d_order, n, d_src, d_dst, d_ws, ws_bytes, d_results,
                                    stream or None)


def plan_sliced(descs, slice_bytes, kernel="auto"):
    """LzmaGpu_PlanSliced: fills descs' probs_off; returns (SlicedPlan, order)."""
    n = len(descs)
    order = (ctypes.c_uint32 * max(n, 1))()
    p = SlicedPlan()
    r = _lib.LzmaGpu_PlanSliced(descs, n, slice_bytes, SLICED_KERNELS[kernel], order,
                                ctypes.byref(p))
    if r != SZ_OK:
        raise RuntimeError(f"LzmaGpu_PlanSliced failed: {r}")
    return p, order


def decode_batch_sliced_device(plan, d_descs, d_order, d_src, d_dst, d_ws, d_results,
                               first_round=0, n_rounds=0, stream=0):
    """LzmaGpu_DecodeBatchSliced over raw device pointers (ints)."""
    return _lib.LzmaGpu_DecodeBatchSliced(ctypes.byref(plan), d_descs, d_order, d_src, d_dst,
                                          d_ws, d_results, first_round, n_rounds, stream or None)


def sliced_active(plan, d_ws, round_, stream=0):
    """Streams still unfinished entering round `round_` (synchronises `stream`)."""
    v = ctypes.c_size_t(0)
    r = _lib.LzmaGpu_SlicedActive(ctypes.byref(plan), d_ws, round_, ctypes.byref(v), stream or None)
    if r != SZ_OK:
        raise RuntimeError(f"LzmaGpu_SlicedActive failed: {r}")
    return v.value


def decode_batch_sliced_host(descs, src, dst_bytes, slice_bytes, kernel="auto", plan_out=None):
    """Time-sliced batch from host buffers: (res, results[ctypes], dst bytes)."""
    n = len(descs)
    res = (Result * max(n, 1))()
    s = _buf(src)
    d = ctypes.create_string_buffer(max(dst_bytes, 1))
    r = _lib.LzmaGpu_DecodeBatchSlicedHost(descs, n, s, len(src), d, dst_bytes, res, slice_bytes,
                                           SLICED_KERNELS[kernel],
                                           ctypes.byref(plan_out) if plan_out is not None else None)
    return r, res, d.raw[:dst_bytes]


def split_lzma2_blocks(src):
    """Lzma2Gpu_SplitBlocks: list of (src_off, src_len, unpack) per dict-reset block."""
    cap = max(16, len(src) // 16)
    s = _buf(src)
    while True:
        o = (ctypes.c_uint64 * cap)()
        ln = (ctypes.c_uint64 * cap)()
        u = (ctypes.c_uint64 * cap)()
        nb = _lib.Lzma2Gpu_SplitBlocks(s, len(src), o, ln, u, cap)
        if nb == ctypes.c_size_t(-1).value:
            raise ValueError("malformed LZMA2 chunk headers")
        if nb <= cap:
            return [(o[i], ln[i], u[i]) for i in range(nb)]
        cap = nb


# ---------------------------------------------------------------- CRC-32 (7zCrc.h)

CRC_CHUNK = 2048  # kCrcChunk in csrc/crc_device.h (CRC-32 and CRC-64)


def CrcCalc(data):
    """7zCrc.c CrcCalc on the GPU (host buffer in, CRC out)."""
    return _lib.CrcCalc(_buf(data), len(data))


def CrcUpdate(crc, data):
    """7zCrc.c CrcUpdate (raw register, no final XOR) on the GPU."""
    return _lib.CrcUpdate(crc, _buf(data), len(data))


def crc_plan(caps):
    """CrcGpu_PlanChunks: (chunk_base[n], chunk_range[n_chunks]) as ctypes arrays."""
    n = len(caps)
    c = (ctypes.c_uint64 * max(n, 1))(*caps)
    total = _lib.CrcGpu_PlanChunks(c, n, None, None)
    if total == ctypes.c_size_t(-1).value:
        raise ValueError("too many CRC chunks")
    base = (ctypes.c_uint32 * max(n, 1))()
    rng = (ctypes.c_uint32 * max(total, 1))()
    _lib.CrcGpu_PlanChunks(c, n, base, rng)
    return base, rng, total


def crc32_plan_decoded(descs):
    """LzmaGpu_Crc32Plan over planned decode descriptors (host)."""
    n = len(descs)
    total = _lib.LzmaGpu_Crc32Plan(descs, n, None, None)
    base = (ctypes.c_uint32 * max(n, 1))()
    rng = (ctypes.c_uint32 * max(total, 1))()
    _lib.LzmaGpu_Crc32Plan(descs, n, base, rng)
    return base, rng, total


def crc_batch_device(d_data, d_off, d_len, n, d_base, d_range, n_chunks, init, xorout,
                     d_chunk_crc, d_crc, stream=0):
    """CrcGpu_Batch over raw device pointers (ints)."""
    return _lib.CrcGpu_Batch(d_data, d_off, d_len, n, d_base, d_range, n_chunks, init, xorout,
                             d_chunk_crc, d_crc, stream or None)


def crc32_batch_decoded(d_descs, d_results, n, d_dst, d_base, d_range, n_chunks, d_chunk_crc,
                        d_crc, stream=0):
    """LzmaGpu_Crc32Batch over raw device pointers (ints)."""
    return _lib.LzmaGpu_Crc32Batch(d_descs, d_results, n, d_dst, d_base, d_range, n_chunks,
                                   d_chunk_crc, d_crc, stream or None)


# ---------------------------------------------------------------- xz, x86 BCJ, CRC-64

def x86_Convert(data, ip=0, state=0, encoding=0):
    """Bra86.c x86_Convert on the GPU: (processed, state, converted bytes)."""
    b = ctypes.create_string_buffer(bytes(data), max(len(data), 1))
    st = ctypes.c_uint32(state)
    n = _lib.x86_Convert(b, len(data), ip, ctypes.byref(st), encoding)
    return n, st.value, b.raw[:len(data)]


BRA_KINDS = {"PPC": 5, "IA64": 6, "ARM": 7, "ARMT": 8, "SPARC": 9}


def bra_convert(kind, data, ip=0, encoding=0):
    """Bra.c / BraIA64.c <kind>_Convert on the GPU: (processed, converted bytes)."""
    b = ctypes.create_string_buffer(bytes(data), max(len(data), 1))
    n = getattr(_lib, kind + "_Convert")(b, len(data), ip, encoding)
    return n, b.raw[:len(data)]


def delta_convert(data, delta, state=b"", encoding=0):
    """Delta.c Delta_Decode (encoding 0) / Delta_Encode on the GPU: (state, bytes)."""
    st = ctypes.create_string_buffer(bytes(state).ljust(256, b"\0")[:256], 256)
    b = ctypes.create_string_buffer(bytes(data), max(len(data), 1))
    (_lib.Delta_Encode if encoding else _lib.Delta_Decode)(st, delta, b, len(data))
    return st.raw, b.raw[:len(data)]


def bra_batch_device(kind, d_data, d_off, d_len, d_ip, d_done, n, encoding=0, stream=0):
    """BraGpu_Batch over raw device pointers (ints)."""
    return _lib.BraGpu_Batch(kind, d_data, d_off, d_len, d_ip, d_done, n, encoding, stream or None)


def delta_batch_device(d_data, d_off, d_len, d_delta, d_state, n, encoding=0, stream=0):
    """DeltaGpu_Batch over raw device pointers (ints)."""
    return _lib.DeltaGpu_Batch(d_data, d_off, d_len, d_delta, d_state, n, encoding, stream or None)


def Bcj2_Decode(main, call, jump, rc, out_size, overlap=False, fill=0xA5):
    """Bcj2.c Bcj2_Decode on the GPU over host buffers: (res, output buffer).
    The output buffer starts as `fill` bytes; overlap: the main stream sits at
    its tail (the 7zDec.c:367-372 layout)."""
    out = ctypes.create_string_buffer(bytes([fill]) * max(out_size, 1), max(out_size, 1))
    bufs = [_buf(x) for x in (call, jump, rc)]
    if overlap:
        at = out_size - len(main)
        ctypes.memmove(ctypes.addressof(out) + at, bytes(main), len(main))
        m = ctypes.addressof(out) + at
    else:
        mb = _buf(main)
        m = ctypes.addressof(mb)
    r = _lib.Bcj2_Decode(m, len(main), bufs[0], len(call), bufs[1], len(jump), bufs[2], len(rc),
                         out, out_size)
    return r, out.raw[:out_size]


def bcj2_batch_device(d_jobs, n, d_res, stream=0):
    """Bcj2Gpu_Batch over a device array of n Bcj2Job."""
    return _lib.Bcj2Gpu_Batch(d_jobs, n, d_res, stream or None)


def bcj2_bound(n):
    """Bcj2EncGpu_Bound: capacities for main, call, jump, rc that hold any n bytes."""
    b = (ctypes.c_uint64 * 4)()
    _lib.Bcj2EncGpu_Bound(n, b)
    return list(b)


def bcj2_scratch(descs, n):
    """Bcj2EncGpu_Scratch: the scratch bytes of a batch of n Bcj2EncDesc."""
    return _lib.Bcj2EncGpu_Scratch(descs, n)


def bcj2_encode_batch_device(d_descs, n, d_src, d_dst, d_scratch, d_results, stream=0):
    """Bcj2EncGpu_EncodeBatch over raw device pointers (ints)."""
    return _lib.Bcj2EncGpu_EncodeBatch(d_descs, n, d_src, d_dst, d_scratch, d_results,
                                       stream or None)


def bcj2_encode_batch_host(descs, n, src, dst, workspace_limit=0):
    """Bcj2EncGpu_EncodeBatchHost: dst (bytes) is the output buffer's initial
    contents.  Returns (res, results[ctypes], dst bytes after the call)."""
    res = (Bcj2EncResult * max(n, 1))()
    d = ctypes.create_string_buffer(bytes(dst), max(len(dst), 1))
    r = _lib.Bcj2EncGpu_EncodeBatchHost(descs, n, _buf(src), len(src), d, len(dst), res,
                                        workspace_limit)
    return r, res, d.raw[:len(dst)]


def bcj2_encode(data):
    """The four BCJ2 streams of x86 code: (main, call, jump, rc), a branch
    converted when its target lies inside `data`."""
    cap = bcj2_bound(len(data))
    desc = (Bcj2EncDesc * 1)()
    desc[0].src_len = len(data)
    at = 0
    for k in range(4):
        desc[0].out[k].off, desc[0].out[k].cap = at, cap[k]
        at += cap[k]
    r, res, out = bcj2_encode_batch_host(desc, 1, data, bytes(at))
    if r != 0 or res[0].res != 0:
        raise RuntimeError("bcj2_encode: res %d / %d: %s" % (r, res[0].res, last_error()))
    return tuple(out[desc[0].out[k].off:desc[0].out[k].off + res[0].len[k]] for k in range(4))


def Crc64Calc(data):
    """XzCrc64.c Crc64Calc on the GPU."""
    return _lib.Crc64Calc(_buf(data), len(data))


def bcj_x86_batch_device(d_data, d_off, d_len, d_ip, d_state, d_done, n, encoding=0, stream=0):
    """BcjGpu_X86Batch over raw device pointers (ints)."""
    return _lib.BcjGpu_X86Batch(d_data, d_off, d_len, d_ip, d_state, d_done, n, encoding,
                                stream or None)


def crc64_batch_device(d_data, d_off, d_len, n, d_base, d_range, n_chunks, init, xorout,
                       d_chunk_crc, d_crc, stream=0):
    """Crc64Gpu_Batch over raw device pointers (ints)."""
    return _lib.Crc64Gpu_Batch(d_data, d_off, d_len, n, d_base, d_range, n_chunks, init, xorout,
                               d_chunk_crc, d_crc, stream or None)


SHA256_DIGEST_SIZE = 32
SHA256_AUTO, SHA256_LANE, SHA256_WAVE = 0, 1, 2  # LZMA_GPU_SHA256_*


def Sha256_Init(p):
    """Sha256.c Sha256_Init on a CSha256."""
    _lib.Sha256_Init(ctypes.byref(p))


def Sha256_Update(p, data):
    """Sha256.c Sha256_Update: whole blocks are compressed on the GPU, the rest buffered."""
    _lib.Sha256_Update(ctypes.byref(p), _buf(data), len(data))


def Sha256_Final(p):
    """Sha256.c Sha256_Final: the 32 digest bytes; p is re-initialised."""
    out = ctypes.create_string_buffer(SHA256_DIGEST_SIZE)
    _lib.Sha256_Final(ctypes.byref(p), out)
    return out.raw


def Sha256(data):
    """SHA-256 of a host buffer through the drop-ins (GPU compute)."""
    p = CSha256()
    Sha256_Init(p)
    Sha256_Update(p, data)
    return Sha256_Final(p)


def sha256_batch_device(d_data, d_off, d_len, n, d_digest, kernel=SHA256_AUTO, stream=0):
    """Sha256Gpu_Batch over raw device pointers (ints); d_digest: n x 32 bytes."""
    return _lib.Sha256Gpu_Batch(d_data, d_off, d_len, n, kernel, d_digest, stream or None)


def xz_index(data):
    """LzmaGpu_XzIndex: (res, [XzBlock...], unpack_total).  Host only."""
    n = ctypes.c_size_t(0)
    tot = ctypes.c_uint64(0)
    src = _buf(data)
    r = _lib.LzmaGpu_XzIndex(src, len(data), None, 0, ctypes.byref(n), ctypes.byref(tot))
    if r != SZ_OK:
        return r, [], 0
    arr = (XzBlock * max(n.value, 1))()
    r = _lib.LzmaGpu_XzIndex(src, len(data), arr, n.value, ctypes.byref(n), ctypes.byref(tot))
    return r, list(arr)[:n.value], tot.value


def XzDecode(data, dest_cap):
    """LzmaGpu_XzDecode: (res, output bytes, bad_block)."""
    out = ctypes.create_string_buffer(max(dest_cap, 1))
    dl = ctypes.c_size_t(dest_cap)
    bad = ctypes.c_int64(-1)
    r = _lib.LzmaGpu_XzDecode(out, ctypes.byref(dl), _buf(data), len(data), ctypes.byref(bad))
    return r, out.raw[:dl.value], bad.value


SZ_PPMD = 1  # LZMA_GPU_7Z_PPMD: method 0x030401 folders decode (off: SZ_ERROR_UNSUPPORTED)


def sz_open(data, flags=0):
    """LzmaGpu_7zOpenEx: (res, [SzFolder...], [SzFile...], names (UTF-16LE bytes),
    unpack_total).  A packed header is decoded on the GPU.  flags: SZ_PPMD."""
    nfo, nfi, nn = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    tot = ctypes.c_uint64(0)
    src = _buf(data)
    r = _lib.LzmaGpu_7zOpenEx(src, len(data), None, 0, ctypes.byref(nfo), None, 0,
                              ctypes.byref(nfi), None, 0, ctypes.byref(nn), ctypes.byref(tot),
                              flags)
    if r != SZ_OK:
        return r, [], [], b"", 0
    fo = (SzFolder * max(nfo.value, 1))()
    fi = (SzFile * max(nfi.value, 1))()
    names = (ctypes.c_uint16 * max(nn.value, 1))()
    r = _lib.LzmaGpu_7zOpenEx(src, len(data), fo, nfo.value, ctypes.byref(nfo), fi, nfi.value,
                              ctypes.byref(nfi), names, nn.value, ctypes.byref(nn),
                              ctypes.byref(tot), flags)
    raw = bytes(bytearray(ctypes.string_at(names, 2 * nn.value)))
    return r, list(fo)[:nfo.value], list(fi)[:nfi.value], raw, tot.value


def SzExtract(data, dest_cap, max_files=1 << 16, flags=0):
    """LzmaGpu_7zExtractEx: (res, extraction buffer, [per-file SRes]).  flags: SZ_PPMD."""
    out = ctypes.create_string_buffer(max(dest_cap, 1))
    dl = ctypes.c_size_t(dest_cap)
    fres = (ctypes.c_int * max_files)()
    r = _lib.LzmaGpu_7zExtractEx(out, ctypes.byref(dl), _buf(data), len(data), fres, max_files,
                                 flags)
    return r, out.raw[:dl.value], list(fres)


# ---------------------------------------------------------------- 7z writing

SZ_ITEM_DIR, SZ_ITEM_JOIN = 1, 2
SZ_WRITE_ENCODE_HEADER, SZ_WRITE_TIMINGS = 1, 2
SZ_STAGES = ("upload", "crc", "filter", "encode", "pack", "download", "header", "total")
SZ_HEADER_STUB = 1
SZ_M_COPY, SZ_M_LZMA, SZ_M_LZMA2, SZ_M_PPMD = 0, 0x030101, 0x21, 0x030401
SZ_FILTER_X86, SZ_FILTER_ARM, SZ_FILTER_BCJ2 = 4, 7, 0x1B
SZ_PACK_COPY, SZ_PACK_LZMA, SZ_PACK_LZMA2, SZ_PACK_PPMD = 0, 1, 2, 3
SZ_PACK_LAST = 1


def sz_method(method=SZ_M_LZMA, filter=0, level=1, dict_size=0, lc=-1, lp=-1, pb=-1,
              block_size=0, order=6, mem_size=1 << 20):
    """One LzmaGpu7zMethod row: the LZMA / LZMA2 props as enc2_props gives them."""
    m = SzMethod()
    m.method, m.filter, m.ppmd_order, m.ppmd_mem_size = method, filter, order, mem_size
    m.props = enc2_props(level, dict_size, lc, lp, pb, block_size)
    return m


def sz_items(entries):
    """entries: (name, src_off, size, flags, method index).  Returns the SzItem
    array and the names buffer (a ctypes uint16 array, NUL after every name)."""
    arr = (SzItem * max(len(entries), 1))()
    units = []
    for i, (name, off, size, flags, method) in enumerate(entries):
        raw = name.encode("utf-16-le")
        u = [int.from_bytes(raw[k:k + 2], "little") for k in range(0, len(raw), 2)] + [0]
        it = arr[i]
        it.src_off, it.size, it.flags, it.method = off, size, flags, method
        it.name_off, it.name_len = len(units), len(u)
        units += u
    names = (ctypes.c_uint16 * max(len(units), 1))(*units)
    return arr, names, len(units)


def _array(ctype, rows):
    arr = (ctype * max(len(rows), 1))()
    for i, r in enumerate(rows):
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(r), ctypes.sizeof(ctype))
    return arr


def sz_write_plan(items, n, src_size, names_len, methods):
    """LzmaGpu_7zWritePlan: (res, [SzFolder...], n_pieces, dest_bound)."""
    marr = _array(SzMethod, methods)
    nfo, npc = ctypes.c_size_t(0), ctypes.c_size_t(0)
    bound = ctypes.c_uint64(0)
    args = (items, n, src_size, names_len, marr, len(methods))
    r = _lib.LzmaGpu_7zWritePlan(*args, None, 0, ctypes.byref(nfo), ctypes.byref(npc),
                                 ctypes.byref(bound))
    if r != SZ_OK:
        return r, [], 0, 0
    fo = (SzFolder * max(nfo.value, 1))()
    r = _lib.LzmaGpu_7zWritePlan(*args, fo, nfo.value, ctypes.byref(nfo), ctypes.byref(npc),
                                 ctypes.byref(bound))
    return r, list(fo)[:nfo.value], npc.value, bound.value


def sz_write_header(folders, items, n, file_crcs, names, names_len, flags=0, pack_area_size=0):
    """LzmaGpu_7zWriteHeader: (res, header bytes, the 32-byte signature header)."""
    farr = _array(SzFolder, folders)
    crcs = (ctypes.c_uint32 * max(n, 1))(*file_crcs) if file_crcs is not None else None
    hl = ctypes.c_size_t(0)
    sig = ctypes.create_string_buffer(32)
    r = _lib.LzmaGpu_7zWriteHeader(farr, len(folders), items, n, crcs, names, names_len, flags,
                                   None, 0, ctypes.byref(hl), None, 0)
    if r != SZ_ERROR_OUTPUT_EOF:
        return r, b"", b""
    out = ctypes.create_string_buffer(max(hl.value, 1))
    r = _lib.LzmaGpu_7zWriteHeader(farr, len(folders), items, n, crcs, names, names_len, flags,
                                   out, hl.value, ctypes.byref(hl), sig, pack_area_size)
    return r, out.raw[:hl.value], sig.raw


def sz_write_header_ex(folders, items, n, file_crcs, names, names_len, bcj2, flags=0,
                       pack_area_size=0):
    """LzmaGpu_7zWriteHeaderEx: bcj2 = one SzBcj2Info per four-coder folder, in
    order.  (res, header bytes, the 32-byte signature header)."""
    farr = _array(SzFolder, folders)
    barr = _array(SzBcj2Info, bcj2)
    crcs = (ctypes.c_uint32 * max(n, 1))(*file_crcs) if file_crcs is not None else None
    hl = ctypes.c_size_t(0)
    sig = ctypes.create_string_buffer(32)
    args = (farr, len(folders), items, n, crcs, names, names_len, flags, barr, len(bcj2))
    r = _lib.LzmaGpu_7zWriteHeaderEx(*args, None, 0, ctypes.byref(hl), None, 0)
    if r != SZ_ERROR_OUTPUT_EOF:
        return r, b"", b""
    out = ctypes.create_string_buffer(max(hl.value, 1))
    r = _lib.LzmaGpu_7zWriteHeaderEx(*args, out, hl.value, ctypes.byref(hl), sig, pack_area_size)
    return r, out.raw[:hl.value], sig.raw


def SzWrite(src, items, n, names, names_len, methods, dest_cap, flags=0, workspace_limit=0,
            fill=0):
    """LzmaGpu_7zWrite: (res, destLen, the whole dest buffer, SzWriteStats)."""
    marr = _array(SzMethod, methods)
    opt = SzWriteOptions(flags, 0, workspace_limit)
    st = SzWriteStats()
    d = ctypes.create_string_buffer(bytes([fill]) * max(dest_cap, 1), max(dest_cap, 1))
    dl = ctypes.c_size_t(dest_cap)
    r = _lib.LzmaGpu_7zWrite(d, ctypes.byref(dl), _buf(src), len(src), items, n, names, names_len,
                             marr, len(methods), ctypes.byref(opt), ctypes.byref(st))
    return r, dl.value, d.raw[:dest_cap], st


def sz_pack_scratch(n):
    return _lib.SzGpu_PackScratch(n)


def sz_pack_batch_device(args, stream=0):
    """SzGpu_PackBatch over an SzPackArgs of raw device pointers (ints)."""
    return _lib.SzGpu_PackBatch(ctypes.byref(args), stream or None)


def sevenz_compress(files, method=SZ_M_LZMA, filter=0, solid=0, encode_header=False, level=1,
                    dict_size=0, block_size=0, order=6, mem_size=1 << 20):
    """A 7z archive of `files`, (name, bytes | None) pairs (None: a directory),
    every file with data a folder of its own, or `solid` files per folder.
    Returns the archive bytes; raises on an error."""
    entries, src, run = [], bytearray(), 0
    for name, data in files:
        if data is None:
            entries.append((name, 0, 0, SZ_ITEM_DIR, 0))
            continue
        join = SZ_ITEM_JOIN if (len(data) and solid > 1 and run % solid) else 0
        entries.append((name, len(src), len(data), join, 0))
        if len(data):
            run += 1
        src += data
    items, names, names_len = sz_items(entries)
    methods = [sz_method(method, filter, level, dict_size, block_size=block_size, order=order,
                         mem_size=mem_size)]
    r, _, _, bound = sz_write_plan(items, len(entries), len(src), names_len, methods)
    if r != SZ_OK:
        raise RuntimeError(f"LzmaGpu_7zWritePlan: {r}: {last_error()}")
    flags = SZ_WRITE_ENCODE_HEADER if encode_header else 0
    r, n, out, _ = SzWrite(bytes(src), items, len(entries), names, names_len, methods, bound, flags)
    if r != SZ_OK:
        raise RuntimeError(f"LzmaGpu_7zWrite: {r}: {last_error()}")
    return out[:n]


# ---------------------------------------------------------------- PPMd7 batches

def ppmd7_workspace_bytes(mem_size):
    """One stream's workspace slice (a multiple of 256 bytes; 0 for a bad mem_size)."""
    return _lib.Ppmd7Gpu_WorkspaceBytes(mem_size)


def ppmd7_make_descs(items):
    """items: dicts with src_off, src_len, dst_off, dst_len, order, mem_size and
    optionally ws_off.  Returns a ctypes Ppmd7StreamDesc array."""
    arr = (Ppmd7StreamDesc * max(len(items), 1))()
    for i, it in enumerate(items):
        d = arr[i]
        d.src_off, d.src_len = it["src_off"], it["src_len"]
        d.dst_off, d.dst_len = it["dst_off"], it["dst_len"]
        d.ws_off = it.get("ws_off", 0)
        d.mem_size, d.order = it["mem_size"], it["order"]
    return arr


def ppmd7_decode_batch_device(d_descs, n, d_src, d_dst, d_ws, d_results, stream=0):
    """Ppmd7Gpu_DecodeBatch over raw device pointers (ints)."""
    return _lib.Ppmd7Gpu_DecodeBatch(d_descs, n, d_src, d_dst, d_ws, d_results, stream or None)


def ppmd7_decode_batch_host(descs, n, src, dst, workspace_limit=0):
    """Ppmd7Gpu_DecodeBatchHost: dst (bytes) is the output buffer's initial
    contents.  Returns (res, results[ctypes], dst bytes after the call)."""
    res = (Ppmd7Result * max(n, 1))()
    d = ctypes.create_string_buffer(bytes(dst), max(len(dst), 1))
    r = _lib.Ppmd7Gpu_DecodeBatchHost(descs, n, _buf(src), len(src), d, len(dst), res,
                                      workspace_limit)
    return r, res, d.raw[:len(dst)]


def ppmd7_make_enc_descs(items):
    """items: dicts with src_off, src_len, dst_off, dst_cap, order, mem_size and
    optionally ws_off.  Returns a ctypes Ppmd7EncDesc array."""
    arr = (Ppmd7EncDesc * max(len(items), 1))()
    for i, it in enumerate(items):
        d = arr[i]
        d.src_off, d.src_len = it["src_off"], it["src_len"]
        d.dst_off, d.dst_cap = it["dst_off"], it["dst_cap"]
        d.ws_off = it.get("ws_off", 0)
        d.mem_size, d.order = it["mem_size"], it["order"]
    return arr


def ppmd7_encode_batch_device(d_descs, n, d_src, d_dst, d_ws, d_results, stream=0):
    """Ppmd7Gpu_EncodeBatch over raw device pointers (ints)."""
    return _lib.Ppmd7Gpu_EncodeBatch(d_descs, n, d_src, d_dst, d_ws, d_results, stream or None)


def ppmd7_encode_batch_host(descs, n, src, dst, workspace_limit=0):
    """Ppmd7Gpu_EncodeBatchHost: dst (bytes) is the output buffer's initial
    contents.  Returns (res, results[ctypes], dst bytes after the call)."""
    res = (Ppmd7EncResult * max(n, 1))()
    d = ctypes.create_string_buffer(bytes(dst), max(len(dst), 1))
    r = _lib.Ppmd7Gpu_EncodeBatchHost(descs, n, _buf(src), len(src), d, len(dst), res,
                                      workspace_limit)
    return r, res, d.raw[:len(dst)]


# ---------------------------------------------------------------- streaming sessions

# ---------------------------------------------------------------- LZMA encoding

SZ_ERROR_OUTPUT_EOF = 7


def enc_props(level=1, dict_size=0, lc=-1, lp=-1, pb=-1, fb=-1, mc=0, algo=-1, bt_mode=-1):
    """A CLzmaEncProps after LzmaEncProps_Init with the given fields set."""
    p = CLzmaEncProps()
    _lib.LzmaEncProps_Init(ctypes.byref(p))
    p.level, p.dictSize, p.lc, p.lp, p.pb, p.fb, p.mc = level, dict_size, lc, lp, pb, fb, mc
    p.algo, p.btMode = algo, bt_mode
    return p


def enc_desc_from_props(props, end_mark=False):
    """LzmaEncGpu_DescFromProps: (res, EncStreamDesc, props5)."""
    d = EncStreamDesc()
    props5 = ctypes.create_string_buffer(5)
    r = _lib.LzmaEncGpu_DescFromProps(ctypes.byref(props), 1 if end_mark else 0, ctypes.byref(d),
                                      props5)
    return r, d, props5.raw


ENC_MODE_OPTIMAL, ENC_MODE_BT4 = 1, 2


def enc_set_modes(allowed):
    """LzmaEncGpu_SetModes: the process-wide mask of normal modes (ENC_MODE_*)
    that the props entry points may select; returns the previous mask."""
    return _lib.LzmaEncGpu_SetModes(allowed)


def enc_get_modes():
    return _lib.LzmaEncGpu_GetModes()


def enc_desc_from_props_ex(props, allowed, end_mark=False):
    """LzmaEncGpu_DescFromPropsEx: (res, EncStreamDesc, props5)."""
    d = EncStreamDesc()
    props5 = ctypes.create_string_buffer(5)
    r = _lib.LzmaEncGpu_DescFromPropsEx(ctypes.byref(props), 1 if end_mark else 0, allowed,
                                        ctypes.byref(d), props5)
    return r, d, props5.raw


def enc_plan(descs, n):
    """LzmaEncGpu_PlanBatch: fills descs[i].ws_off; (res, order, workspace_bytes)."""
    order = (ctypes.c_uint32 * max(n, 1))()
    ws = ctypes.c_uint64(0)
    r = _lib.LzmaEncGpu_PlanBatch(descs, n, order, ctypes.byref(ws))
    return r, list(order)[:n], ws.value


def encode_batch_device(d_descs, d_order, n, d_src, d_dst, d_ws, d_results, lanes=0, stream=0):
    """LzmaEncGpu_EncodeBatch over raw device pointers (ints)."""
    return _lib.LzmaEncGpu_EncodeBatch(d_descs, d_order or None, n, d_src, d_dst, d_ws, d_results,
                                       lanes, stream or None)


def encode_batch_host(descs, n, src, dst, workspace_limit=0):
    """LzmaEncGpu_EncodeBatchHost: dst (bytes) is the output buffer's initial
    contents.  Returns (res, results, dst bytes)."""
    res = (EncResult * max(n, 1))()
    d = ctypes.create_string_buffer(bytes(dst), max(len(dst), 1))
    r = _lib.LzmaEncGpu_EncodeBatchHost(descs, n, _buf(src), len(src), d, len(dst), res,
                                        workspace_limit)
    return r, res, d.raw[:len(dst)]


def encode_batch(items, level=1, dict_size=0, lc=-1, lp=-1, pb=-1, fb=-1, mc=0, end_mark=False):
    """Encodes every bytes object of `items` with the same props in one host
    batch.  Returns [(res, props5, packed)] per item; the capacity of each item
    is len + len / 2 + 1024.  Props outside the fast path give
    (SZ_ERROR_UNSUPPORTED or SZ_ERROR_PARAM, b"", b"") for every item."""
    r, proto, props5 = enc_desc_from_props(enc_props(level, dict_size, lc, lp, pb, fb, mc), end_mark)
    if r != SZ_OK:
        return [(r, b"", b"")] * len(items)
    n = len(items)
    descs = (EncStreamDesc * max(n, 1))()
    src_off = dst_off = 0
    for i, it in enumerate(items):
        ctypes.memmove(ctypes.byref(descs[i]), ctypes.byref(proto), ctypes.sizeof(proto))
        cap = len(it) + len(it) // 2 + 1024
        descs[i].src_off, descs[i].src_len, descs[i].dst_off, descs[i].dst_cap = (
            src_off, len(it), dst_off, cap)
        src_off += len(it)
        dst_off += cap
    r, res, out = encode_batch_host(descs, n, b"".join(bytes(it) for it in items), bytes(dst_off))
    if r != SZ_OK:
        return [(r, b"", b"")] * n
    return [(res[i].res, props5, out[descs[i].dst_off:descs[i].dst_off + res[i].dest_len])
            for i in range(n)]


def LzmaEncode(src, props, dest_cap, end_mark=False, props_size=5):
    """The drop-in: (res, destLen, props bytes, packed bytes)."""
    d = ctypes.create_string_buffer(max(dest_cap, 1))
    dl = ctypes.c_size_t(dest_cap)
    pe = ctypes.create_string_buffer(8)
    ps = ctypes.c_size_t(props_size)
    res = _lib.LzmaEncode(d, ctypes.byref(dl), _buf(src), len(src), ctypes.byref(props), pe,
                          ctypes.byref(ps), 1 if end_mark else 0, None, None, None)
    ok = res in (SZ_OK, SZ_ERROR_OUTPUT_EOF)
    return res, dl.value, pe.raw[:5], d.raw[:dl.value] if ok else b""


def LzmaCompress(src, dest_cap, level=5, dict_size=0, lc=-1, lp=-1, pb=-1, fb=-1, num_threads=1):
    """The drop-in: (res, destLen, props bytes, packed bytes)."""
    d = ctypes.create_string_buffer(max(dest_cap, 1))
    dl = ctypes.c_size_t(dest_cap)
    pe = ctypes.create_string_buffer(8)
    ps = ctypes.c_size_t(5)
    res = _lib.LzmaCompress(d, ctypes.byref(dl), _buf(src), len(src), pe, ctypes.byref(ps), level,
                            dict_size, lc, lp, pb, fb, num_threads)
    ok = res in (SZ_OK, SZ_ERROR_OUTPUT_EOF)
    return res, dl.value, pe.raw[:5], d.raw[:dl.value] if ok else b""


# ---------------------------------------------------------------- LZMA encoder sessions

ENC_SESSION_HOLD = 546
ENC_SESSION_NEEDS_INPUT, ENC_SESSION_FINISHED, ENC_SESSION_BUDGET = 0, 1, 2
SZ_ERROR_READ, SZ_ERROR_WRITE, SZ_ERROR_PROGRESS = 8, 9, 10


def enc_session_workspace_bytes(props, src_cap):
    """LzmaEncGpu_SessionWorkspaceBytes."""
    return _lib.LzmaEncGpu_SessionWorkspaceBytes(ctypes.byref(props), src_cap)


def enc_session_init(s, props, d_src, src_cap, d_dst, dst_cap, d_ws, end_mark=False):
    """LzmaEncGpu_SessionInit into the EncSession s (device pointers as ints):
    (res, props5)."""
    props5 = ctypes.create_string_buffer(5)
    r = _lib.LzmaEncGpu_SessionInit(ctypes.byref(s), ctypes.byref(props), 1 if end_mark else 0,
                                    d_src or None, src_cap, d_dst or None, dst_cap, d_ws or None,
                                    props5)
    return r, props5.raw


def enc_session_scratch_bytes(n):
    return _lib.LzmaEncGpu_SessionScratchBytes(n)


def enc_session_encode_batch(d_sessions, n, d_scratch, lanes=0, stream=0):
    """LzmaEncGpu_SessionEncodeBatch over a device array of n EncSessions."""
    return _lib.LzmaEncGpu_SessionEncodeBatch(d_sessions, n, d_scratch, lanes, stream or None)


def enc_session_list_pass(d_sessions, n, d_scratch, stream=0):
    """The round's list pass alone (lzmaenc_session_bench.py)."""
    return _lib.LzmaEncGpu_SessionListPass(d_sessions, n, d_scratch, stream or None)


class LzmaEncSessions:
    """n encoder sessions on torch device tensors: one
    source, destination and workspace slab each, cut evenly; the records live
    on the device and are mirrored here.

        s = LzmaEncSessions(n, src_cap, dst_cap, level=1)   # or props=[...] per session
        s.append(i, piece)        # any number of sessions, any piece sizes
        s.round(finish=[...])     # one LzmaEncGpu_SessionEncodeBatch
        s.drain(i)                # the bytes of session i that are new

    After round(), s.rec[i] holds res / status / in_pos / out_pos."""

    def __init__(self, n, src_cap, dst_cap, end_mark=False, device="cuda", props=None,
                 dst_caps=None, poison=None, **kw):
        """props: one CLzmaEncProps or a list of n (default: enc_props(**kw));
        end_mark: one flag or a list of n; dst_caps: per-session capacities at
        most dst_cap (the slot size); poison: a byte the destination and the
        workspace are filled with first."""
        import torch
        self.torch, self.n, self.src_cap, self.dst_cap = torch, n, src_cap, dst_cap
        plist = list(props) if isinstance(props, (list, tuple)) else [props or enc_props(**kw)] * n
        marks = list(end_mark) if isinstance(end_mark, (list, tuple)) else [end_mark] * n
        caps = list(dst_caps) if dst_caps is not None else [dst_cap] * n
        self.ws_bytes = [enc_session_workspace_bytes(p, src_cap) for p in plist]
        if any(b == 0 for b in self.ws_bytes):
            raise ValueError("props or src_cap refused: " + last_error())
        self.ws_off = [sum(self.ws_bytes[:i]) for i in range(n)]

        def slab(nbytes, fill=None):
            if fill is None:
                return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
            return torch.full((max(nbytes, 16),), fill, dtype=torch.uint8, device=device)
        self.src, self.dst = slab(n * src_cap), slab(n * dst_cap, poison)
        self.ws = slab(sum(self.ws_bytes), poison)
        self.scratch = slab(enc_session_scratch_bytes(n))
        self.rec = (EncSession * max(n, 1))()
        self.props5 = [b""] * n
        for i in range(n):
            r, self.props5[i] = enc_session_init(
                self.rec[i], plist[i], self.src.data_ptr() + i * src_cap, src_cap,
                self.dst.data_ptr() + i * dst_cap, caps[i], self.ws.data_ptr() + self.ws_off[i],
                marks[i])
            if r != SZ_OK:
                raise ValueError("LzmaEncGpu_SessionInit: %d %s" % (r, last_error()))
        self.d_rec = slab(ctypes.sizeof(self.rec))
        self.supplied = [0] * n
        self.drained = [0] * n
        self._upload()

    def _host(self):
        return self.torch.frombuffer(self.rec, dtype=self.torch.uint8)

    def _upload(self):
        self.d_rec[:ctypes.sizeof(self.rec)].copy_(self._host())

    def append(self, i, piece):
        """Appends piece (bytes) to session i's source on the device."""
        if not piece:
            return
        at = self.supplied[i]
        assert at + len(piece) <= self.src_cap
        t = self.torch.frombuffer(bytearray(piece), dtype=self.torch.uint8)
        self.src[i * self.src_cap + at:i * self.src_cap + at + len(piece)].copy_(t)
        self.supplied[i] = at + len(piece)

    def round(self, finish=(), in_budget=0, lanes=0, sync=True):
        """One round over all n sessions; finish: indices whose stream is
        complete.  Returns LzmaEncGpu_SessionEncodeBatch's result."""
        fin = set(finish)
        for i in range(self.n):
            self.rec[i].src_len = self.supplied[i]
            self.rec[i].finish = 1 if i in fin else 0
            self.rec[i].in_budget = in_budget
        self._upload()
        r = enc_session_encode_batch(self.d_rec.data_ptr(), self.n, self.scratch.data_ptr(), lanes,
                                     self.torch.cuda.current_stream().cuda_stream)
        if sync:
            self.download()
        return r

    def download(self):
        self._host().copy_(self.d_rec[:ctypes.sizeof(self.rec)])

    def worked(self):
        """Sessions the last round listed as having work (scratch word 0)."""
        return int(self.scratch[:4].view(self.torch.int32)[0])

    def drain(self, i):
        """dst[drained, out_pos) of session i: the bytes not yet taken."""
        upto = min(self.rec[i].out_pos, self.rec[i].dst_cap)
        lo = self.drained[i]
        self.drained[i] = upto
        return bytes(self.dst[i * self.dst_cap + lo:i * self.dst_cap + upto].cpu().numpy())


def LzmaEnc_Encode(read, write, props, progress=None):
    """The handle drop-ins end to end: Create, SetProps, WriteProperties, Encode
    over Python callables -- read(n) -> bytes (b"" at the end), write(b) -> count
    taken, progress(in, out) -> 0 to go on -- and Destroy.  (res, props5)."""
    h = _lib.LzmaEnc_Create(ctypes.byref(g_alloc))
    try:
        r = _lib.LzmaEnc_SetProps(h, ctypes.byref(props))
        if r != SZ_OK:
            return r, b""
        p5 = ctypes.create_string_buffer(5)
        ps = ctypes.c_size_t(5)
        r = _lib.LzmaEnc_WriteProperties(h, p5, ctypes.byref(ps))
        if r != SZ_OK:
            return r, b""

        def _read(_p, buf, size):
            b = read(size[0])
            ctypes.memmove(buf, b, len(b))
            size[0] = len(b)
            return SZ_OK

        def _write(_p, buf, size):
            return write(ctypes.string_at(buf, size))
        ins, outs = ISeqInStream(SeqRead(_read)), ISeqOutStream(SeqWrite(_write))
        prog = ICompressProgress(ProgressFn(lambda _p, a, b: progress(a, b))) if progress else None
        r = _lib.LzmaEnc_Encode(h, ctypes.byref(outs), ctypes.byref(ins),
                                ctypes.byref(prog) if prog else None, None, None)
        return r, p5.raw
    finally:
        _lib.LzmaEnc_Destroy(h, ctypes.byref(g_alloc), ctypes.byref(g_alloc))


def LzmaEnc_MemEncode(src, props, dest_cap, end_mark=False):
    """LzmaEnc_Create / SetProps / MemEncode / Destroy: (res, packed)."""
    h = _lib.LzmaEnc_Create(ctypes.byref(g_alloc))
    try:
        r = _lib.LzmaEnc_SetProps(h, ctypes.byref(props))
        if r != SZ_OK:
            return r, b""
        d = ctypes.create_string_buffer(max(dest_cap, 1))
        dl = ctypes.c_size_t(dest_cap)
        r = _lib.LzmaEnc_MemEncode(h, d, ctypes.byref(dl), _buf(src), len(src),
                                   1 if end_mark else 0, None, None, None)
        return r, d.raw[:dl.value] if r in (SZ_OK, SZ_ERROR_OUTPUT_EOF) else b""
    finally:
        _lib.LzmaEnc_Destroy(h, ctypes.byref(g_alloc), ctypes.byref(g_alloc))


# ---------------------------------------------------------------- LZMA2 and xz writing

def enc2_props(level=1, dict_size=0, lc=-1, lp=-1, pb=-1, block_size=0, block_threads=-1,
               total_threads=-1, lzma_threads=-1):
    """A CLzma2EncProps after Lzma2EncProps_Init with the given fields set."""
    p = CLzma2EncProps()
    _lib.Lzma2EncProps_Init(ctypes.byref(p))
    q = p.lzmaProps
    q.level, q.dictSize, q.lc, q.lp, q.pb, q.numThreads = level, dict_size, lc, lp, pb, lzma_threads
    p.blockSize, p.numBlockThreads, p.numTotalThreads = block_size, block_threads, total_threads
    return p


def block_bound(n):
    return _lib.Lzma2EncGpu_BlockBound(n)


def enc2_desc_from_props(props):
    """Lzma2EncGpu_DescFromProps: (res, EncStreamDesc, prop byte)."""
    d = EncStreamDesc()
    prop = ctypes.c_ubyte(0)
    r = _lib.Lzma2EncGpu_DescFromProps(ctypes.byref(props), ctypes.byref(d), ctypes.byref(prop))
    return r, d, prop.value


def enc2_desc_from_props_ex(props, allowed):
    """Lzma2EncGpu_DescFromPropsEx: (res, EncStreamDesc, prop byte)."""
    d = EncStreamDesc()
    prop = ctypes.c_ubyte(0)
    r = _lib.Lzma2EncGpu_DescFromPropsEx(ctypes.byref(props), allowed, ctypes.byref(d),
                                         ctypes.byref(prop))
    return r, d, prop.value


def enc2_plan(descs, n):
    """Lzma2EncGpu_PlanBatch: fills descs[i].ws_off; (res, order, workspace_bytes)."""
    order = (ctypes.c_uint32 * max(n, 1))()
    ws = ctypes.c_uint64(0)
    r = _lib.Lzma2EncGpu_PlanBatch(descs, n, order, ctypes.byref(ws))
    return r, list(order)[:n], ws.value


def lzma2_encode_batch_device(d_descs, d_order, n, d_src, d_dst, d_ws, d_results, lanes=0,
                              stream=0):
    """Lzma2EncGpu_EncodeBatch over raw device pointers (ints)."""
    return _lib.Lzma2EncGpu_EncodeBatch(d_descs, d_order or None, n, d_src, d_dst, d_ws, d_results,
                                        lanes, stream or None)


def lzma2_compact_device(d_descs, d_results, n, d_slots, d_out, out_cap, d_offsets, d_total,
                         stream=0):
    """Lzma2EncGpu_Compact over raw device pointers (ints)."""
    return _lib.Lzma2EncGpu_Compact(d_descs, d_results, n, d_slots, d_out, out_cap, d_offsets,
                                    d_total, stream or None)


def lzma2_encode_batch_host(descs, n, src, dst, workspace_limit=0):
    """Lzma2EncGpu_EncodeBatchHost: dst (bytes) is the output buffer's initial
    contents.  Returns (res, results, dst bytes)."""
    res = (EncResult * max(n, 1))()
    d = ctypes.create_string_buffer(bytes(dst), max(len(dst), 1))
    r = _lib.Lzma2EncGpu_EncodeBatchHost(descs, n, _buf(src), len(src), d, len(dst), res,
                                         workspace_limit)
    return r, res, d.raw[:len(dst)]


def lzma2_encode_batch(items, level=1, dict_size=0, lc=-1, lp=-1, pb=-1):
    """Encodes every bytes object of `items` as one LZMA2 block (chunks from a
    dictionary reset on, no final 0x00) with the same props in one host batch.
    Returns [(res, prop, packed)] per item; each item's capacity is its block
    bound."""
    r, proto, prop = enc2_desc_from_props(enc2_props(level, dict_size, lc, lp, pb))
    if r != SZ_OK:
        return [(r, 0, b"")] * len(items)
    n = len(items)
    descs = (EncStreamDesc * max(n, 1))()
    src_off = dst_off = 0
    for i, it in enumerate(items):
        ctypes.memmove(ctypes.byref(descs[i]), ctypes.byref(proto), ctypes.sizeof(proto))
        cap = block_bound(len(it))
        descs[i].src_off, descs[i].src_len, descs[i].dst_off, descs[i].dst_cap = (
            src_off, len(it), dst_off, cap)
        src_off += len(it)
        dst_off += cap
    r, res, out = lzma2_encode_batch_host(descs, n, b"".join(bytes(it) for it in items),
                                          bytes(dst_off))
    if r != SZ_OK:
        return [(r, 0, b"")] * n
    return [(res[i].res, prop, out[descs[i].dst_off:descs[i].dst_off + res[i].dest_len])
            for i in range(n)]


def Lzma2EncodeHost(src, props, dest_cap):
    """LzmaGpu_Lzma2EncodeHost: (res, prop byte, stream bytes)."""
    d = ctypes.create_string_buffer(max(dest_cap, 1))
    dl = ctypes.c_size_t(dest_cap)
    prop = ctypes.c_ubyte(0)
    r = _lib.LzmaGpu_Lzma2EncodeHost(d, ctypes.byref(dl), _buf(src), len(src), ctypes.byref(props),
                                     ctypes.byref(prop))
    return r, prop.value, d.raw[:dl.value] if r == SZ_OK else b""


def lzma2_compress(data, level=1, dict_size=0, block_size=0, lc=-1, lp=-1, pb=-1):
    """One LZMA2 stream (blocks of block_size, 0 = the reference's default) and
    its dictionary byte: (prop, bytes).  Raises on an error."""
    bs = block_size or (1 << 20)    # the default block is 1 MiB or more
    cap = len(data) + 1 + (len(data) // bs + 1) * (block_bound(bs) - bs)
    r, prop, out = Lzma2EncodeHost(data, enc2_props(level, dict_size, lc, lp, pb, block_size), cap)
    if r != SZ_OK:
        raise RuntimeError(f"LzmaGpu_Lzma2EncodeHost: {r}: {last_error()}")
    return prop, out


def XzEncode(src, props, check, dest_cap):
    """LzmaGpu_XzEncode: (res, file bytes)."""
    d = ctypes.create_string_buffer(max(dest_cap, 1))
    dl = ctypes.c_size_t(dest_cap)
    r = _lib.LzmaGpu_XzEncode(d, ctypes.byref(dl), _buf(src), len(src), ctypes.byref(props), check)
    return r, d.raw[:dl.value] if r == SZ_OK else b""


def xz_filters(chain):
    """[(id, prop)] as an XzFilter array (None for an empty chain) and its length."""
    chain = list(chain)
    if not chain:
        return None, 0
    arr = (XzFilter * len(chain))()
    for k, (fid, prop) in enumerate(chain):
        arr[k].id, arr[k].prop = fid, prop
    return arr, len(chain)


def XzEncodeEx(src, props, check, dest_cap, chain=()):
    """LzmaGpu_XzEncodeEx with chain = [(id, prop)]: (res, file bytes)."""
    d = ctypes.create_string_buffer(max(dest_cap, 1))
    dl = ctypes.c_size_t(dest_cap)
    arr, k = xz_filters(chain)
    r = _lib.LzmaGpu_XzEncodeEx(d, ctypes.byref(dl), _buf(src), len(src), ctypes.byref(props),
                                check, arr, k)
    return r, d.raw[:dl.value] if r == SZ_OK else b""


def xz_compress(data, check=1, level=1, dict_size=0, block_size=0, lc=-1, lp=-1, pb=-1, chain=()):
    """One xz stream, a block per block_size bytes, chain = [(id, prop)] in front
    of LZMA2.  Raises on an error."""
    bs = block_size or (1 << 20)
    blocks = len(data) // bs + 1
    cap = 64 + len(data) + blocks * (block_bound(bs) - bs + 12 + 4 + 32 + 20 + 24)
    r, out = XzEncodeEx(data, enc2_props(level, dict_size, lc, lp, pb, block_size), check, cap,
                        chain)
    if r != SZ_OK:
        raise RuntimeError(f"LzmaGpu_XzEncodeEx: {r}: {last_error()}")
    return out


# ---------------------------------------------------------------- Lzma86

LZMA86_HEADER_SIZE = 14
SZ_FILTER_NO, SZ_FILTER_YES, SZ_FILTER_AUTO = 0, 1, 2
LZMA86_TIMINGS = 1


def lzma86_descs(items):
    """items: dicts with src_off, src_len, dst_off, dst_cap and, for encoding,
    level, dict_size, mode."""
    arr = (Lzma86StreamDesc * max(len(items), 1))()
    for i, it in enumerate(items):
        arr[i].src_off, arr[i].src_len = it["src_off"], it["src_len"]
        arr[i].dst_off, arr[i].dst_cap = it["dst_off"], it["dst_cap"]
        arr[i].level, arr[i].dictSize = it.get("level", 1), it.get("dict_size", 0)
        arr[i].filterMode = it.get("mode", SZ_FILTER_AUTO)
    return arr


def lzma86_encode_scratch(descs, n):
    b = ctypes.c_uint64(0)
    r = _lib.Lzma86Gpu_EncodeScratch(descs, n, ctypes.byref(b))
    return r, b.value


def lzma86_encode_batch_device(descs, n, d_src, d_dst, d_scratch, scratch_bytes, d_results,
                               stream=0):
    """Lzma86Gpu_EncodeBatch: descs on the host, the rest raw device pointers (ints)."""
    return _lib.Lzma86Gpu_EncodeBatch(descs, n, d_src, d_dst, d_scratch, scratch_bytes, d_results,
                                      stream or None)


def lzma86_encode_batch_host(descs, n, src, dst, workspace_limit=0, stats=None):
    """Lzma86Gpu_EncodeBatchHost: dst (bytes) is the output buffer's initial
    contents.  Returns (res, results, dst bytes)."""
    res = (Lzma86Result * max(n, 1))()
    d = ctypes.create_string_buffer(bytes(dst), max(len(dst), 1))
    r = _lib.Lzma86Gpu_EncodeBatchHost(descs, n, _buf(src), len(src), d, len(dst), res,
                                       workspace_limit,
                                       ctypes.byref(stats) if stats is not None else None)
    return r, res, d.raw[:len(dst)]


def lzma86_headers(descs, n, src):
    """The 14 header bytes per stream the decode calls take, from the host copy."""
    out = bytearray(14 * max(n, 1))
    for i in range(n):
        h = src[descs[i].src_off:descs[i].src_off + min(14, descs[i].src_len)]
        out[14 * i:14 * i + len(h)] = h
    return bytes(out)


def lzma86_decode_scratch(descs, n, headers):
    b = ctypes.c_uint64(0)
    r = _lib.Lzma86Gpu_DecodeScratch(descs, n, headers, ctypes.byref(b))
    return r, b.value


def lzma86_decode_batch_device(descs, n, headers, d_src, d_dst, d_scratch, scratch_bytes,
                               d_results, stream=0):
    return _lib.Lzma86Gpu_DecodeBatch(descs, n, headers, d_src, d_dst, d_scratch, scratch_bytes,
                                      d_results, stream or None)


def lzma86_decode_batch_host(descs, n, src, dst):
    res = (Lzma86Result * max(n, 1))()
    d = ctypes.create_string_buffer(bytes(dst), max(len(dst), 1))
    r = _lib.Lzma86Gpu_DecodeBatchHost(descs, n, _buf(src), len(src), d, len(dst), res)
    return r, res, d.raw[:len(dst)]


def Lzma86_Encode(src, dest_cap, level=1, dict_size=0, mode=SZ_FILTER_AUTO):
    """The drop-in: (res, destLen, stream bytes)."""
    d = ctypes.create_string_buffer(max(dest_cap, 1))
    dl = ctypes.c_size_t(dest_cap)
    res = _lib.Lzma86_Encode(d, ctypes.byref(dl), _buf(src), len(src), level, dict_size, mode)
    return res, dl.value, d.raw[:dl.value]


def Lzma86_GetUnpackSize(src):
    v = ctypes.c_uint64(0)
    res = _lib.Lzma86_GetUnpackSize(_buf(src), len(src), ctypes.byref(v))
    return res, v.value


def Lzma86_Decode(src, dest_cap):
    """The drop-in: (res, destLen, srcLen, bytes)."""
    d = ctypes.create_string_buffer(max(dest_cap, 1))
    dl = ctypes.c_size_t(dest_cap)
    sl = ctypes.c_size_t(len(src))
    res = _lib.Lzma86_Decode(d, ctypes.byref(dl), _buf(src), ctypes.byref(sl))
    return res, dl.value, sl.value, d.raw[:dl.value] if res == SZ_OK else b""


def session_probs_bytes(props):
    return _lib.LzmaGpu_SessionProbsBytes(bytes(props), len(props))


def session_init(props, d_probs, d_dic, dic_buf_size):
    """Host-side LzmaDec_Allocate + LzmaDec_Init on a fresh Session (device pointers in)."""
    s = Session()
    r = _lib.LzmaGpu_SessionInit(ctypes.byref(s), bytes(props), len(props), d_probs, d_dic,
                                 dic_buf_size)
    return r, s


def session_decode_batch(d_sessions, n, stream=0):
    """LzmaGpu_SessionDecodeBatch over a device array of n Sessions."""
    return _lib.LzmaGpu_SessionDecodeBatch(d_sessions, n, stream or None)
