"""Postdata seal, host-only restatement of the format.

Used by the tests to say what the GPU must produce; nothing on the product
path imports it — the engine writes, reads and checks the sidecar itself.

    sealed stream  postdata_0.bin, postdata_1.bin, ... up to the first absent
                   file, floor(size / 16) labels of each, concatenated
    page p         labels [1024 p, min(1024 (p + 1), total)) of the stream
    digest         first 16 bytes of SHA-256 over the page's bytes
    sidecar        postdata_seal.bin: 32-byte little-endian header, then
                   ceil(total / 1024) digests

and of the part files a sealed init leaves until they are assembled (§3.7),
further down.
"""
import hashlib
import os
import struct

MAGIC = b"PSTSEAL1"
PAGE_LABELS = 1024
DIGEST_BYTES = 16
LABEL_SIZE = 16
HEADER = struct.Struct("<8sIIQQ")
HEADER_SIZE = HEADER.size           # 32
SIDECAR = "postdata_seal.bin"


def num_pages(total_labels: int) -> int:
    return -(-total_labels // PAGE_LABELS)


def pack_header(total_labels: int, page_labels: int = PAGE_LABELS,
                digest_bytes: int = DIGEST_BYTES, magic: bytes = MAGIC,
                reserved: int = 0) -> bytes:
    return HEADER.pack(magic, page_labels, digest_bytes, total_labels,
                       reserved)


def unpack_header(buf: bytes) -> dict:
    """The header's fields; ValueError for what the engine refuses too."""
    if len(buf) < HEADER_SIZE:
        raise ValueError("shorter than the header")
    magic, page_labels, digest_bytes, total, reserved = HEADER.unpack_from(buf)
    if magic != MAGIC:
        raise ValueError("wrong magic")
    if page_labels != PAGE_LABELS or digest_bytes != DIGEST_BYTES:
        raise ValueError("unsupported page_labels or digest_bytes")
    return {"page_labels": page_labels, "digest_bytes": digest_bytes,
            "total_labels": total, "reserved": reserved}


def page_digests(data: bytes) -> bytes:
    """Digests of the pages of a label stream, back to back.  Trailing bytes
    short of a whole label are not part of the stream."""
    total = len(data) // LABEL_SIZE
    page = PAGE_LABELS * LABEL_SIZE
    view = memoryview(data)[:total * LABEL_SIZE]
    return b"".join(
        hashlib.sha256(view[o:o + page]).digest()[:DIGEST_BYTES]
        for o in range(0, len(view), page))


def read_stream(data_dir: str) -> bytes:
    """The sealed stream of a dir, as the proving pass reads it."""
    out = []
    i = 0
    while True:
        path = os.path.join(data_dir, f"postdata_{i}.bin")
        if not os.path.exists(path):
            break
        with open(path, "rb") as f:
            raw = f.read()
        out.append(raw[:len(raw) // LABEL_SIZE * LABEL_SIZE])
        i += 1
    return b"".join(out)


def sidecar_bytes(data: bytes) -> bytes:
    """What postdata_seal.bin holds for a label stream."""
    return pack_header(len(data) // LABEL_SIZE) + page_digests(data)


# Seal during init: a session over [index_start, index_end)
# appends its digests to postdata_seal.part-<index_start>:
#
#     header  32 bytes little-endian: magic PSTSEALP, page_labels,
#             digest_bytes, first_page u64, end_page u64 (exclusive)
#     body    one digest per closed page, in page order

PART_MAGIC = b"PSTSEALP"
PART_PREFIX = "postdata_seal.part-"


def part_name(index_start: int) -> str:
    return f"{PART_PREFIX}{index_start}"


def pack_part_header(first_page: int, end_page: int,
                     page_labels: int = PAGE_LABELS,
                     digest_bytes: int = DIGEST_BYTES,
                     magic: bytes = PART_MAGIC) -> bytes:
    return HEADER.pack(magic, page_labels, digest_bytes, first_page, end_page)


def unpack_part_header(buf: bytes) -> dict:
    if len(buf) < HEADER_SIZE:
        raise ValueError("shorter than the header")
    magic, page_labels, digest_bytes, first, end = HEADER.unpack_from(buf)
    if magic != PART_MAGIC:
        raise ValueError("wrong magic")
    if page_labels != PAGE_LABELS or digest_bytes != DIGEST_BYTES:
        raise ValueError("unsupported page_labels or digest_bytes")
    return {"page_labels": page_labels, "digest_bytes": digest_bytes,
            "first_page": first, "end_page": end}


def part_bytes(data: bytes, index_start: int, index_end: int,
               pages_done=None) -> bytes:
    """The part file of the shard [index_start, index_end) of the stream
    `data`, with its first pages_done digests (all by default)."""
    first = index_start // PAGE_LABELS
    end = num_pages(index_end)
    body = page_digests(data[index_start * LABEL_SIZE:
                             index_end * LABEL_SIZE])
    if pages_done is not None:
        body = body[:pages_done * DIGEST_BYTES]
    return pack_part_header(first, end) + body


def stream_digests(data: bytes, cuts=(), stream_end: bool = True) -> bytes:
    """Digests of a stream that is hashed in segments cut at `cuts`.  Where
    the cuts fall must not matter, so this is page_digests; without
    stream_end a ragged last page stays open and has no digest."""
    total = len(data) // LABEL_SIZE
    assert all(0 <= c <= total for c in cuts)
    out = page_digests(data)
    return out if stream_end else out[:total // PAGE_LABELS * DIGEST_BYTES]
