"""Re-cut a BAM into small record-aligned BGZF blocks (test helper, no GPU, no product decoder).

The device decoder takes a chunk only if it holds at least 64 BGZF blocks (csrc/bam.cpp schedule_chunk), so the golden BAMs - at most
10,000 records in 64 KB blocks - never reach it.  The same records in many small blocks do, at a small XCK_CHUNK_BYTES, and a reader
that is independent of the product (oracle/pybam.py: gzip + the BAM specification) does not care how a file is blocked: what the
unmodified reference wrote for the original file is the expected output for the re-cut one.

The source is read with `gzip` and cut at the records' block_size fields; the blocks are written with the synthetic-input
writer's bgzf_block / BGZF_EOF (zlib).  Nothing here calls into csrc/."""
import gzip
import os
import shutil
import struct
import zlib

from xcltk_amd.synth import bamwriter

_CONSUMES_REF = (1, 0, 1, 1, 0, 0, 0, 1, 1, 0)                          # MIDNSHP=X (SAMv1 section 1.4.6)


def split_bam(src):
    """-> (header bytes: magic, text and reference list; [record bytes, block_size field included]) of a BAM file, read with gzip"""
    with gzip.open(src, "rb") as fp:
        d = fp.read()
    assert d[:4] == b"BAM\x01", src
    l_text, = struct.unpack_from("<i", d, 4)
    off = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, off)
    off += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", d, off)
        off += 4 + l_name + 4
    header, recs = d[:off], []
    while off < len(d):
        bs, = struct.unpack_from("<i", d, off)
        assert bs >= 32 and off + 4 + bs <= len(d), "record at %d overruns the file" % off
        recs.append(d[off:off + 4 + bs])
        off += 4 + bs
    return header, recs


def write_blocks(dst, header, recs, sizes, rng, share_header, empty_every=0):
    """header + records -> BGZF file of blocks that hold whole records; see reblock_bam.  -> (n_blocks, [records per block])"""
    out, per_block = [], []

    def put(payload, n_rec):
        out.append(bamwriter.bgzf_block(bytes(payload)))
        per_block.append(n_rec)
        if empty_every and sum(1 for k in per_block if k > 0) % empty_every == 0:
            out.append(bamwriter.bgzf_block(b""))                          # payload of 0 bytes: legal BGZF (the EOF marker is one)
            per_block.append(0)

    buf = bytearray(header)
    while len(buf) > bamwriter.BGZF_MAX_PAYLOAD or (buf and not share_header):
        n = min(len(buf), bamwriter.BGZF_MAX_PAYLOAD - (1 if share_header else 0))      # (shared: the last header block keeps a tail)
        out.append(bamwriter.bgzf_block(bytes(buf[:n])))
        per_block.append(-1)                                               # a header-only block
        del buf[:n]
    i, first = 0, True
    while i < len(recs):
        target = int(sizes[int(rng.integers(0, len(sizes)))])
        base = len(buf) if first else 0                                    # the header's tail does not count against the target
        n = 0
        while i < len(recs) and (n == 0 or len(buf) - base + len(recs[i]) <= target) and len(buf) + len(recs[i]) <= bamwriter.BGZF_MAX_PAYLOAD:
            buf += recs[i]
            i += 1
            n += 1
        assert n > 0, "a record does not fit a BGZF block next to the header's tail"
        put(buf, n)
        buf = bytearray()
        first = False
    if buf:                                                                # (no records at all: the header's tail)
        out.append(bamwriter.bgzf_block(bytes(buf)))
        per_block.append(-1)
    with open(dst, "wb") as fp:
        fp.write(b"".join(out) + bamwriter.BGZF_EOF)
    return len(out) + 1, per_block + [0]                                   # (the EOF marker is the file's last block)


def reblock_bam(src, dst, sizes, rng, share_header, empty_every=0):
    """Write the records of BAM `src` to `dst` as BGZF blocks that each hold whole records.  The payload target of each block is drawn
    from `sizes` with `rng` (numpy Generator); a block takes records while they fit the target, and at least one.  share_header=True
    puts the header's tail and the first records into one block (the first record then starts inside a block: the chunk's first_skip
    is non-zero), False ends the header's block first.  empty_every=k inserts an empty block after every k-th block of records.
    -> (number of records, number of blocks with the EOF marker, most records in one block)"""
    header, recs = split_bam(src)
    n_blocks, per_block = write_blocks(dst, header, recs, sizes, rng, share_header, empty_every)
    return len(recs), n_blocks, max([0] + per_block)


def _rec_span(rec):
    """(tid, pos, end, flag) of a record for the index: end as htslib's bam_endpos"""
    tid, pos, l_name, _mapq, _bin, n_cig, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    cig = struct.unpack_from("<%dI" % n_cig, rec, 36 + l_name)
    rlen = sum(v >> 4 for v in cig if _CONSUMES_REF[v & 15]) if not flag & 4 else 0
    return tid, pos, pos + (rlen or 1), flag


def reblock_bam_indexed(src, dst, block_payload=3000):
    """The records of `src` through BamWriter.write_raw in blocks of `block_payload` bytes, under the source's header text, and the
    .bai that belongs to the re-cut file (BamWriter.write_index).  -> number of records"""
    header, recs = split_bam(src)
    l_text, = struct.unpack_from("<i", header, 4)
    text = header[8:8 + l_text].decode("ascii")
    refs, off = [], 12 + l_text
    while off < len(header):
        l_name, = struct.unpack_from("<i", header, off)
        refs.append((header[off + 4:off + 4 + l_name - 1].decode("ascii"), struct.unpack_from("<i", header, off + 4 + l_name)[0]))
        off += 8 + l_name
    w = bamwriter.BamWriter(dst, refs, header_text=text, block_payload=block_payload)
    for rec in recs:
        w.write_raw(rec, *_rec_span(rec))
    w.close()
    w.write_index()
    return len(recs)


def read_blocks(path):
    """-> [(payload size, payload)] of every BGZF block of a file, the EOF marker included (zlib on each member; SAMv1 section 4.1)"""
    raw = open(path, "rb").read()
    out, at = [], 0
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 12:at + 16] == b"BC\x02\x00", "not a BGZF block at %d" % at
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        payload = zlib.decompress(raw[at + 18:at + bsize - 8], -15)
        assert struct.unpack_from("<II", raw, at + bsize - 8) == (zlib.crc32(payload) & 0xffffffff, len(payload))
        out.append((len(payload), payload))
        at += bsize
    return out


def block_records(path):
    """Records per BGZF block of a record-aligned BAM, as [[(tid, pos), ...] per block from the first block with records on]; asserts
    that no record straddles blocks.  -> (index of the first block with records, bytes of it before the first record, lists)"""
    blocks = read_blocks(path)
    header, _ = split_bam(path)
    left, first = len(header), 0
    while left > 0 and left >= blocks[first][0]:                          # a block of header bytes only
        left -= blocks[first][0]
        first += 1
    out = []
    for k in range(first, len(blocks)):
        p, o, recs = blocks[k][1], (left if k == first else 0), []
        while o < len(p):
            bs, tid, pos = struct.unpack_from("<iii", p, o)
            assert o + 4 + bs <= len(p), "a record straddles blocks"
            recs.append((tid, pos))
            o += 4 + bs
        out.append(recs)
    return first, left, out


def plan_chunks(path, chunk_bytes):
    """The chunks a reader with XCK_CHUNK_BYTES=chunk_bytes cuts a file into (csrc/bam.cpp Scanner::scan: from the first block with
    records on, blocks are added while the chunk's inflated size is below the target).  -> [number of blocks per chunk]"""
    first, _, _ = block_records(path)
    sizes = [n for n, _ in read_blocks(path)][first:]
    chunks, n, usz = [], 0, 0
    for s in sizes:
        n += 1
        usz += s
        if usz >= chunk_bytes:
            chunks.append(n)
            n, usz = 0, 0
    if n:
        chunks.append(n)
    return chunks


def recut_dataset(src_dir, dst_dir, recut):
    """Copy a golden dataset to dst_dir with every BAM re-cut by recut(src bam, dst bam); the .bai files are left out (their virtual
    offsets no longer hold; the single-process front-ends use no index).  -> {bam name: what recut returned}"""
    os.makedirs(dst_dir, exist_ok=True)
    out = {}
    for f in sorted(os.listdir(src_dir)):
        s, d = os.path.join(src_dir, f), os.path.join(dst_dir, f)
        if f.endswith(".bai"):
            continue
        if f.endswith(".bam"):
            out[f] = recut(s, d)
        elif os.path.isdir(s):
            shutil.copytree(s, d)
        else:
            shutil.copy(s, d)
    return out
