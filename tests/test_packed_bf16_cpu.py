"""The surface of the packed forward's bf16 mode that needs no GPU: the option's number in the header and in the Python table,
and the two segment-kernel entry points declared in include/w2v2.h with the argument lists wav2vec2/_native.py binds."""

import ctypes
import os
import re

from wav2vec2 import _native as N
from wav2vec2.modeling import Wav2Vec2Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CTYPES = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}


def header():
    src = open(os.path.join(ROOT, "include", "w2v2.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_option_number_in_header_and_python():
    assert re.search(r"^#define\s+W2V2_OPT_BF16_PACKED\s+5\s*$", header(), flags=re.M)
    assert Wav2Vec2Model.OPTIONS["bf16_packed"] == 5
    assert sorted(Wav2Vec2Model.OPTIONS.values()) == list(range(len(Wav2Vec2Model.OPTIONS)))     # no number taken twice


def declared(name):
    """(return ctype, [argument ctypes]) of `name` as include/w2v2.h declares it; every pointer is a void pointer to ctypes"""
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", header())
    assert m, f"{name} is not declared in include/w2v2.h"
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        if "*" in a:
            args.append(ctypes.c_void_p)
        else:
            args.append(CTYPES[a.replace("const", "").split()[0]])
    return CTYPES[m.group(1)], args


def test_new_ops_are_declared_and_bound_alike():
    for name, nargs in (("w2v2_op_attention_packed_bf16", 9), ("w2v2_op_pos_conv_packed_bf16", 11)):
        res, args = declared(name)
        assert len(args) == nargs
        assert name in N.PROTOTYPES, f"{name} has no ctypes prototype"
        pres, pargs = N.PROTOTYPES[name]
        assert pres is res
        assert list(pargs) == args, name
