"""rv_mosaic_desc as its 37 slots, read from include/rawvae_hip.h and from its ctypes mirror _lib.MosaicDesc.  A slot
that ops read under more than one name is an anonymous union in both; its first member is the slot's own name."""
import os
import re

from conftest import REPO


def header_code():
    """include/rawvae_hip.h without its comments"""
    with open(os.path.join(REPO, "include", "rawvae_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _members(decls):
    """[(name, C type)] of `type a, b; type* c;`"""
    out = []
    for decl in decls.split(";"):
        if decl.strip():
            first, *more = [piece.strip() for piece in decl.split(",")]
            ctype, name = re.fullmatch(r"(.*?)\s*(\w+)", " ".join(first.split())).groups()
            assert all(re.fullmatch(r"\w+", m) for m in more), decl
            out += [(n, ctype) for n in [name] + more]
    return out


def header_slots():
    """One tuple per slot, in declaration order, of its members as (name, C type)"""
    body = re.search(r"typedef struct rv_mosaic_desc \{(.*)\} rv_mosaic_desc;", header_code(), flags=re.S).group(1)
    slots = []
    for union, plain in re.findall(r"union\s*\{(.*?)\}\s*;|([^;{}]+;)", body, flags=re.S):
        slots += [tuple(_members(union))] if union else [(m,) for m in _members(plain)]
    return slots


def ctypes_slots():
    """One tuple per slot, in offset order, of the names _lib.MosaicDesc gives it"""
    from rawaudiovae_kelsey_amd._lib import MosaicDesc
    at = {}
    for name, ctype in MosaicDesc._fields_:
        for n in ([m for m, _ in ctype._fields_] if name in MosaicDesc._anonymous_ else [name]):
            at.setdefault(getattr(MosaicDesc, n).offset, []).append(n)
    return [tuple(at[offset]) for offset in sorted(at)]


def names(slots):
    """header_slots() without the types: comparable with ctypes_slots()"""
    return [tuple(n for n, _ in slot) for slot in slots]


def check_layout():
    """The pins every audio tool's test holds: 37 slots of 8 bytes, the same members in the header and in ctypes.
    Returns the first name of every slot in order: the names a C caller that knows no roles uses."""
    import ctypes
    from rawaudiovae_kelsey_amd._lib import MosaicDesc
    slots = header_slots()
    assert len(slots) == 37 and ctypes.sizeof(MosaicDesc) == 37 * 8
    assert names(slots) == ctypes_slots()
    first = [slot[0][0] for slot in slots]
    assert [getattr(MosaicDesc, n).offset for n in first] == [8 * i for i in range(37)]
    return first
