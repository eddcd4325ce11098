"""Initial proof during init, host-only restatement of the part format
(DESIGN §3.8).

Used by the tests to say what the engine must write and to build the parts
the assembly is tried on; nothing on the product path imports it — the
engine writes, reads and merges the parts itself.

    part     postdata_hits.part-<index_start>, little-endian
    header   128 bytes: magic PSTHITSP, u32 record_bytes = 16, u32 nonces,
             u32 k1, u32 k2, challenge[32], pow_difficulty[32],
             u64 index_start, u64 index_end, u64 total_labels, zeros
    records  16 bytes {u64 index, u32 nonce, u32 tag}: a hit has tag 0; a
             marker has nonce 0xFFFFFFFF, tag 0x4B52414D and index = the
             global index up to which the part is complete
"""
import dataclasses
import struct

MAGIC = b"PSTHITSP"
PART_PREFIX = "postdata_hits.part-"
HEADER = struct.Struct("<8sIIII32s32sQQQ")
HEADER_SIZE = 128
RECORD = struct.Struct("<QII")
RECORD_BYTES = RECORD.size          # 16
MARK_NONCE = 0xFFFFFFFF
MARK_TAG = 0x4B52414D
# what the engine gets with a batch's count before it goes back for more, and
# the bounds of the device buffer of a batch (spacemesh_post.h)
HIT_WINDOW = 1024
HIT_CAP_MIN, HIT_CAP_MAX = 4096, 1 << 16


def part_name(index_start: int) -> str:
    return f"{PART_PREFIX}{index_start}"


def hit_capacity(batch: int, nonces: int, k1: int, total_labels: int) -> int:
    """Records a batch of `batch` labels may have before its step fails."""
    expect = -(-batch * nonces * k1 // total_labels)
    return min(max(16 * expect, HIT_CAP_MIN), HIT_CAP_MAX)


@dataclasses.dataclass
class PartHeader:
    nonces: int
    k1: int
    k2: int
    challenge: bytes
    pow_difficulty: bytes
    index_start: int
    index_end: int
    total_labels: int
    record_bytes: int = RECORD_BYTES
    magic: bytes = MAGIC

    def pack(self) -> bytes:
        raw = HEADER.pack(self.magic, self.record_bytes, self.nonces, self.k1,
                          self.k2, self.challenge, self.pow_difficulty,
                          self.index_start, self.index_end, self.total_labels)
        return raw + bytes(HEADER_SIZE - len(raw))


def unpack_header(buf: bytes) -> PartHeader:
    """The header's fields; ValueError for what the engine refuses too."""
    if len(buf) < HEADER_SIZE:
        raise ValueError("shorter than the header")
    (magic, record_bytes, nonces, k1, k2, challenge, pow_difficulty, start,
     end, total) = HEADER.unpack_from(buf)
    if magic != MAGIC:
        raise ValueError("wrong magic")
    if record_bytes != RECORD_BYTES:
        raise ValueError("unsupported record_bytes")
    return PartHeader(nonces, k1, k2, challenge, pow_difficulty, start, end,
                      total)


def marker(index: int) -> bytes:
    return RECORD.pack(index, MARK_NONCE, MARK_TAG)


def hit(index: int, nonce: int) -> bytes:
    return RECORD.pack(index, nonce, 0)


def build_part(header: PartHeader, hits, marks=None) -> bytes:
    """A part from a hit list [(index, nonce)] (any order) of the header's
    range, with a marker at index_start and one at every index of `marks`
    (default: index_end alone, a finished shard).  Hits at or past the last
    marker are left out, as they are not on disk yet."""
    marks = sorted([header.index_end] if marks is None else marks)
    hits = sorted((int(i), int(n)) for i, n in hits)
    out = [header.pack(), marker(header.index_start)]
    lo = header.index_start
    for m in marks:
        out += [hit(i, n) for i, n in hits if lo <= i < m]
        out.append(marker(m))
        lo = m
    return b"".join(out)


def read_part(buf: bytes):
    """(header, hits, complete_to) of a part: the hits in front of the last
    marker as [(index, nonce)], and that marker's index (index_start when
    there is none).  Trailing bytes short of a record are ignored; a record
    that is out of order ends the reading, as in the engine."""
    h = unpack_header(buf)
    hits, kept, complete_to, last = [], 0, h.index_start, None
    for off in range(HEADER_SIZE, len(buf) - RECORD_BYTES + 1, RECORD_BYTES):
        index, nonce, tag = RECORD.unpack_from(buf, off)
        if nonce == MARK_NONCE and tag == MARK_TAG:
            if index < complete_to or index > h.index_end or \
                    (last is not None and index <= last[0]):
                break
            complete_to, kept = index, len(hits)
        else:
            if tag != 0 or nonce >= h.nonces or index < complete_to or \
                    index >= h.index_end or \
                    (last is not None and (index, nonce) <= last):
                break
            last = (index, nonce)
            hits.append(last)
    return h, hits[:kept], complete_to
