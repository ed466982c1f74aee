"""Child process of tests/test_dropin_tiers.py: LZGPU_MIRROR_BUDGET_MB is read
once per process, so the byte budget of the decoder mirrors is tested in a
fresh one.  16 threads, each in its own LzmaDec_DecodeToBuf loop over a 64 KiB
ring; prints one JSON line: per stream the call count, the trace, the input
used and the SHA-256 of the output, and the path counters."""
import hashlib
import json
import lzma
import os
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lzma-sdk-zliblike_amd"))

THREADS = 16
IN_CHUNK, OUT_CHUNK = 3000, 8192
DICT = 1 << 16


def streams():
    """(plaintext, stream, props) per thread."""
    import lzmaenc_min as E
    import native
    out = []
    for k in range(THREADS):
        data = native.gen("text", 8100 + k, 150_000 + 1000 * k)
        comp = lzma.compress(data, format=lzma.FORMAT_RAW, filters=[
            {"id": lzma.FILTER_LZMA1, "dict_size": DICT, "lc": 3, "lp": 0, "pb": 2}])
        out.append((data, comp, E.props(3, 0, 2, DICT)))
    return out


def main():
    import lzmagpu as L
    if L.device_count() <= 0:
        sys.exit("no HIP device: " + L.last_error())
    ss = streams()
    L.path_stats(reset=True)
    with ThreadPoolExecutor(THREADS) as ex:
        got = list(ex.map(lambda s: L.stream_decode(s[1], s[2], len(s[0]), IN_CHUNK, OUT_CHUNK, 0,
                                                    max_calls=5000), ss))
    runs = [dict(calls=g[0], trace=[list(r) for r in g[1]], used=g[3],
                 sha256=hashlib.sha256(g[2]).hexdigest()) for g in got]
    print(json.dumps(dict(runs=runs, stats=L.path_stats())))


if __name__ == "__main__":
    main()
