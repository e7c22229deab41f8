"""A reader of the vendor-processed reference images of the metamorphic study: single-frame, unsigned, grayscale DICOM files in
little-endian transfer syntaxes, read with numpy and the standard library (the reference reads them with pydicom,
test/metamorphic_test/script.py:396).

read_dicom_gray(path) returns what pydicom's `ds.pixel_array` returns for the files it accepts: the stored values as uint8 or uint16,
shape (Rows, Columns), no modality LUT, no MONOCHROME1 flip. Everything else is refused with a ValueError that names the cause.
"""
import struct

import numpy as np

IMPLICIT_VR_LE = "1.2.840.10008.1.2"
EXPLICIT_VR_LE = "1.2.840.10008.1.2.1"
_REFUSED_SYNTAXES = {"1.2.840.10008.1.2.2": "explicit VR big endian", "1.2.840.10008.1.2.1.99": "deflated explicit VR little endian"}

# explicit VR: these carry a 2-byte reserved field and a 4-byte length, every other VR a 2-byte length (PS3.5 section 7.1.2)
_LONG_VRS = frozenset((b"OB", b"OD", b"OF", b"OL", b"OV", b"OW", b"SQ", b"SV", b"UC", b"UN", b"UR", b"UT", b"UV"))
_UNDEFINED = 0xFFFFFFFF
_ITEM, _ITEM_END, _SEQ_END = (0xFFFE, 0xE000), (0xFFFE, 0xE00D), (0xFFFE, 0xE0DD)
_TRANSFER_SYNTAX = (0x0002, 0x0010)
_PIXEL_DATA = (0x7FE0, 0x0010)
_SAMPLES, _FRAMES, _ROWS, _COLUMNS = (0x0028, 0x0002), (0x0028, 0x0008), (0x0028, 0x0010), (0x0028, 0x0011)
_BITS_ALLOCATED, _STORED_BITS, _PIXEL_REPRESENTATION = (0x0028, 0x0100), (0x0028, 0x0101), (0x0028, 0x0103)


def _tag(t):
    return "(%04X,%04X)" % t


def _header(buf, pos, explicit):
    """The data element header at `pos`: (tag, vr or None, value length, offset of the value)."""
    if pos + 8 > len(buf):
        raise ValueError("truncated data element header at byte %d" % pos)
    tag = struct.unpack_from("<HH", buf, pos)
    if tag[0] == 0xFFFE or not explicit:   # items and delimiters have no VR in either syntax
        return tag, None, struct.unpack_from("<I", buf, pos + 4)[0], pos + 8
    vr = bytes(buf[pos + 4:pos + 6])
    if vr in _LONG_VRS:
        if pos + 12 > len(buf):
            raise ValueError("truncated data element header at byte %d" % pos)
        return tag, vr, struct.unpack_from("<I", buf, pos + 8)[0], pos + 12
    return tag, vr, struct.unpack_from("<H", buf, pos + 6)[0], pos + 8


def _skip_sequence(buf, pos, explicit):
    """`pos`: the value of an element of undefined length (a sequence). Returns the offset after its (FFFE,E0DD)."""
    while True:
        tag, _, length, pos = _header(buf, pos, explicit)
        if tag == _SEQ_END:
            return pos
        if tag != _ITEM:
            raise ValueError("unexpected tag %s inside a sequence of undefined length" % _tag(tag))
        if length == _UNDEFINED:
            _, pos = _dataset(buf, pos, explicit, nested=True)
        elif pos + length > len(buf):
            raise ValueError("truncated sequence item at byte %d" % pos)
        else:
            pos += length


def _dataset(buf, pos, explicit, nested):
    """The data elements from `pos` on. Top level: ({tag: (vr, offset, length)}, end), stopping after PixelData (its length is checked
    against the file by the caller). nested: an item of undefined length, skipped through its (FFFE,E00D); returns ({}, end)."""
    found = {}
    while pos < len(buf):
        tag, vr, length, pos = _header(buf, pos, explicit)
        if nested and tag == _ITEM_END:
            return found, pos
        if length == _UNDEFINED:
            if tag == _PIXEL_DATA and not nested:
                raise ValueError("pixel data %s of undefined length (encapsulated) is not supported" % _tag(tag))
            pos = _skip_sequence(buf, pos, explicit)
            continue
        if not nested:
            found[tag] = (vr, pos, length)
            if tag == _PIXEL_DATA:
                return found, pos + length
        if pos + length > len(buf):
            raise ValueError("truncated element %s at byte %d" % (_tag(tag), pos))
        pos += length
    if nested:
        raise ValueError("sequence item of undefined length without its delimiter (FFFE,E00D)")
    return found, pos


def _us(buf, found, tag, name):
    if tag not in found:
        raise ValueError("missing %s %s" % (name, _tag(tag)))
    _, off, length = found[tag]
    if length < 2:
        raise ValueError("%s %s holds %d bytes, not an unsigned short" % (name, _tag(tag), length))
    return struct.unpack_from("<H", buf, off)[0]


def read_dicom_gray(path):
    """The stored pixel values of a single-frame grayscale DICOM file: uint8 or uint16 of shape (Rows, Columns).

    Accepted: the Part 10 layout (128-byte preamble, 'DICM', file meta group 0002 in explicit VR little endian) with the dataset in
    implicit or explicit VR little endian; sequences and items of defined or undefined length, nested, are skipped; elements of odd
    length are read as they are. Required: Rows, Columns, SamplesPerPixel = 1, BitsAllocated 8 or 16, BitsStored, PixelRepresentation
    = 0, NumberOfFrames absent or 1, and PixelData of defined length covering Rows * Columns values. A stored value above
    2^BitsStored - 1 is refused rather than masked."""
    with open(path, "rb") as f:
        buf = f.read()
    if len(buf) < 132 or buf[128:132] != b"DICM":
        raise ValueError("%s: not a DICOM Part 10 file (no 'DICM' after the 128-byte preamble)" % path)
    pos, meta = 132, {}
    while pos + 8 <= len(buf) and struct.unpack_from("<H", buf, pos)[0] == 0x0002:
        tag, _, length, pos = _header(buf, pos, True)
        if length == _UNDEFINED or pos + length > len(buf):
            raise ValueError("%s: malformed file meta element %s" % (path, _tag(tag)))
        meta[tag] = buf[pos:pos + length]
        pos += length
    if _TRANSFER_SYNTAX not in meta:
        raise ValueError("%s: no TransferSyntaxUID %s in the file meta group" % (path, _tag(_TRANSFER_SYNTAX)))
    uid = meta[_TRANSFER_SYNTAX].rstrip(b"\x00 ").decode("ascii", "replace")
    if uid not in (IMPLICIT_VR_LE, EXPLICIT_VR_LE):
        what = _REFUSED_SYNTAXES.get(uid, "encapsulated (compressed) pixel data")
        raise ValueError("%s: transfer syntax %s (%s) is not supported: only implicit and explicit VR little endian" % (path, uid, what))
    found, _ = _dataset(buf, pos, uid == EXPLICIT_VR_LE, nested=False)

    rows, cols = _us(buf, found, _ROWS, "Rows"), _us(buf, found, _COLUMNS, "Columns")
    samples = _us(buf, found, _SAMPLES, "SamplesPerPixel")
    if samples != 1:
        raise ValueError("%s: colour data (SamplesPerPixel = %d) is not supported" % (path, samples))
    if _FRAMES in found:
        _, off, length = found[_FRAMES]
        text = buf[off:off + length].strip(b"\x00 ")
        try:
            frames = int(text)
        except ValueError:
            raise ValueError("%s: NumberOfFrames %r is not an integer" % (path, text)) from None
        if frames != 1:
            raise ValueError("%s: multi-frame data (NumberOfFrames = %d) is not supported" % (path, frames))
    bits = _us(buf, found, _BITS_ALLOCATED, "BitsAllocated")
    if bits not in (8, 16):
        raise ValueError("%s: BitsAllocated = %d is not supported (8 or 16)" % (path, bits))
    stored = _us(buf, found, _STORED_BITS, "BitsStored")
    if not 1 <= stored <= bits:
        raise ValueError("%s: BitsStored = %d outside [1, BitsAllocated = %d]" % (path, stored, bits))
    signed = _us(buf, found, _PIXEL_REPRESENTATION, "PixelRepresentation")
    if signed != 0:
        raise ValueError("%s: signed data (PixelRepresentation = %d) is not supported" % (path, signed))
    if _PIXEL_DATA not in found:
        raise ValueError("%s: no PixelData %s" % (path, _tag(_PIXEL_DATA)))
    _, off, length = found[_PIXEL_DATA]
    need = rows * cols * (bits // 8)
    if length < need or off + need > len(buf):
        raise ValueError("%s: truncated pixel data: %d bytes for %d x %d values of %d bits" % (path, min(length, len(buf) - off), rows, cols, bits))
    a = np.frombuffer(buf, dtype="<u2" if bits == 16 else np.uint8, count=rows * cols, offset=off).reshape(rows, cols)
    a = a.astype(np.uint16 if bits == 16 else np.uint8)   # native byte order, and a copy the caller owns
    top = int(a.max()) if a.size else 0
    if top > (1 << stored) - 1:
        raise ValueError("%s: stored value %d above 2^BitsStored - 1 = %d" % (path, top, (1 << stored) - 1))
    return a
