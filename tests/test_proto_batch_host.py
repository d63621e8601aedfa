"""tsg_proto_search_batch without a device: the symbol, the whole-call argument errors
(answered before any device work), the empty batch, and the ctypes mirror of tsg_proto_item
against the compiled header."""
import ctypes as C
import os
import subprocess

import tempo_amd as T
from tempo_amd import tsg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def call(ctx, items, n, outs, sts=None):
    return T.lib().tsg_proto_search_batch(ctx, items, n, outs, sts)


def test_symbol_is_exported():
    assert hasattr(T.lib(), "tsg_proto_search_batch")
    assert "tsg_proto_search_batch" in tsg.EXPORTED


def test_invalid_arguments_need_no_device():
    one = (tsg._ProtoItem * 1)()
    outs = (C.POINTER(tsg._ProtoResult) * 1)()
    ctx = C.c_void_p(1)  # (never dereferenced: every case below is refused first)
    blk = C.c_void_p(1)
    req = tsg._ProtoRequest()
    assert call(None, one, 1, outs) == tsg.TSG_E_INVALID      # no context
    assert call(None, None, 0, None) == tsg.TSG_E_INVALID     # ... even for an empty batch
    assert call(ctx, None, 1, outs) == tsg.TSG_E_INVALID      # n > 0 without items
    assert call(ctx, one, 1, None) == tsg.TSG_E_INVALID       # n > 0 without outs
    one[0].block, one[0].req = None, C.addressof(req)
    assert call(ctx, one, 1, outs) == tsg.TSG_E_INVALID       # an item without a block
    one[0].block, one[0].req = blk, None
    assert call(ctx, one, 1, outs) == tsg.TSG_E_INVALID       # an item without a request
    req.ntags = 2                                             # tags announced, arrays NULL
    one[0].block, one[0].req = blk, C.addressof(req)
    assert call(ctx, one, 1, outs) == tsg.TSG_E_INVALID
    # a bad item anywhere refuses the whole call: the valid first item is not run
    two = (tsg._ProtoItem * 2)()
    ok = tsg._ProtoRequest()
    two[0].block, two[0].req = blk, C.addressof(ok)
    two[1].block, two[1].req = blk, None
    outs2 = (C.POINTER(tsg._ProtoResult) * 2)()
    sts = (C.c_int32 * 2)(77, 77)
    assert call(ctx, two, 2, outs2, sts) == tsg.TSG_E_INVALID
    assert list(sts) == [77, 77] and not outs2[0] and not outs2[1]


def test_empty_batch_is_ok():
    ctx = C.c_void_p(1)
    assert call(ctx, None, 0, None) == tsg.TSG_OK
    outs = (C.POINTER(tsg._ProtoResult) * 1)()
    assert call(ctx, (tsg._ProtoItem * 1)(), 0, outs, (C.c_int32 * 1)()) == tsg.TSG_OK


def test_proto_item_layout_matches_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsg.h"\nint main(void){printf("%zu %zu %zu %zu\\n",'
                   ' sizeof(tsg_proto_item), offsetof(tsg_proto_item, block), offsetof(tsg_proto_item, req),'
                   ' sizeof(tsg_proto_request));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(tsg._ProtoItem), tsg._ProtoItem.block.offset, tsg._ProtoItem.req.offset,
                   C.sizeof(tsg._ProtoRequest)]
