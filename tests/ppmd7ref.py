"""The reference's PPMd7 decoder (Ppmd7.c / Ppmd7Dec.c as compiled into
oracle/_ref/libref.so), driven from Python through its exported Ppmd7_*
functions with ctypes callbacks: the byte reader, loop and result rules of
SzDecodePpmd (7zDec.c:66-122) over a memory buffer.  No reference header is
needed: CPpmd7 is an opaque, generously sized block, and the range decoder
(three function pointers, Range, Code, the stream pointer) is laid out here."""
import ctypes

import native

_ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
_FREE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p)
_READ_FN = ctypes.CFUNCTYPE(ctypes.c_ubyte, ctypes.c_void_p)


class _ISzAlloc(ctypes.Structure):
    _fields_ = [("Alloc", _ALLOC_FN), ("Free", _FREE_FN)]


class _IByteIn(ctypes.Structure):
    _fields_ = [("Read", _READ_FN)]


class _RangeDec(ctypes.Structure):
    _fields_ = [("GetThreshold", ctypes.c_void_p), ("Decode", ctypes.c_void_p),
                ("DecodeBit", ctypes.c_void_p), ("Range", ctypes.c_uint32),
                ("Code", ctypes.c_uint32), ("Stream", ctypes.POINTER(_IByteIn))]


_libc = ctypes.CDLL(None)
_libc.malloc.restype = ctypes.c_void_p
_libc.malloc.argtypes = [ctypes.c_size_t]
_libc.free.argtypes = [ctypes.c_void_p]


def _lib():
    lib = native.ref_cont()
    if not getattr(lib, "_ppmd7_declared", False):
        lib.Ppmd7_Construct.argtypes = [ctypes.c_void_p]
        lib.Ppmd7_Alloc.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        lib.Ppmd7_Alloc.restype = ctypes.c_int
        lib.Ppmd7_Free.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.Ppmd7_Init.argtypes = [ctypes.c_void_p, ctypes.c_uint]
        lib.Ppmd7z_RangeDec_CreateVTable.argtypes = [ctypes.c_void_p]
        lib.Ppmd7z_RangeDec_Init.argtypes = [ctypes.c_void_p]
        lib.Ppmd7z_RangeDec_Init.restype = ctypes.c_int
        lib.Ppmd7_DecodeSymbol.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.Ppmd7_DecodeSymbol.restype = ctypes.c_int
        lib._ppmd7_declared = True
    return lib


def decode(packed, order, mem_size, dst_len):
    """(res, dest_len, src_len, written bytes) as SzDecodePpmd over `packed`."""
    if not (2 <= order <= 64 and (1 << 11) <= mem_size <= 0xFFFFFFFF - 36):
        return 4, 0, 0, b""
    lib = _lib()
    alloc = _ISzAlloc(_ALLOC_FN(lambda p, n: _libc.malloc(n)), _FREE_FN(lambda p, a: _libc.free(a)))
    state = {"pos": 0, "extra": False}
    n = len(packed)

    def read(_):
        if state["pos"] < n:
            state["pos"] += 1
            return packed[state["pos"] - 1]
        state["extra"] = True
        return 0

    stream = _IByteIn(_READ_FN(read))
    model = ctypes.create_string_buffer(64 << 10)  # CPpmd7 is about 19 KiB
    rc = _RangeDec()
    lib.Ppmd7_Construct(model)
    assert lib.Ppmd7_Alloc(model, mem_size, ctypes.byref(alloc))
    try:
        lib.Ppmd7_Init(model, order)
        lib.Ppmd7z_RangeDec_CreateVTable(ctypes.byref(rc))
        rc.Stream = ctypes.pointer(stream)
        out = bytearray()
        if not lib.Ppmd7z_RangeDec_Init(ctypes.byref(rc)) or state["extra"]:
            return 1, 0, state["pos"], b""
        while len(out) < dst_len:
            sym = lib.Ppmd7_DecodeSymbol(model, ctypes.byref(rc))
            if state["extra"] or sym < 0:
                break
            out.append(sym)
        ok = len(out) == dst_len and state["pos"] == n and rc.Code == 0
        return (0 if ok else 1), len(out), state["pos"], bytes(out)
    finally:
        lib.Ppmd7_Free(model, ctypes.byref(alloc))
