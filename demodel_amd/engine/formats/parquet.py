"""Parquet page extraction for GPU decompression (BASELINE.json config 5:
c4-en parquet streaming).

A parquet file's column chunks are sequences of pages, each preceded by a
Thrift compact-protocol PageHeader giving the compressed/uncompressed
sizes.  The heavy bytes are the page payloads; the headers are tiny.  So:
CPU walks the headers (this module — a minimal Thrift compact reader, no
parquet library in the data path), and the GPU decompresses every page
payload in one wave-parallel zstd/deflate launch into the HBM ring.

Scope: the full pyarrow codec matrix — ZSTD (csrc/zstd_kernel.hip),
SNAPPY (csrc/snappy.hip, parquet's default codec), GZIP (member header
parsed on CPU, raw DEFLATE on csrc/inflate.hip) and UNCOMPRESSED
(device copy) — for BOTH v1 and v2 data pages (v2 rep+def level
prefixes device-copy; only the values region feeds the codec kernel).
Unknown codecs fail loudly.

Column decode: the decompressed pages are still parquet-encoded (level
streams, PLAIN or dictionary-index values).  plan_columns() /
decode_columns_gpu() take them to typed column tensors in HBM
(csrc/parquet_decode.hip) — see decode_columns_gpu for what is covered.
"""

from __future__ import annotations

from dataclasses import dataclass

# Thrift compact protocol type ids
_CT_STOP = 0
_CT_TRUE = 1
_CT_FALSE = 2
_CT_BYTE = 3
_CT_I16 = 4
_CT_I32 = 5
_CT_I64 = 6
_CT_DOUBLE = 7
_CT_BINARY = 8
_CT_LIST = 9
_CT_SET = 10
_CT_MAP = 11
_CT_STRUCT = 12


class _Compact:
    def __init__(self, data, pos=0):
        self.d = data
        self.p = pos

    def byte(self):
        b = self.d[self.p]
        self.p += 1
        return b

    def _need(self, n: int) -> None:
        # untrusted input: a declared element count beyond the
        # remaining bytes would spin a near-infinite skip loop
        if n < 0 or n > len(self.d) - self.p:
            raise ValueError(
                f"thrift: declared {n} elements with "
                f"{len(self.d) - self.p} bytes left")

    def skip_elem(self, ctype):
        """Skip one LIST/SET/MAP element: unlike struct FIELDS, bool
        elements are encoded as one byte in the compact protocol."""
        if ctype in (_CT_TRUE, _CT_FALSE):
            self.byte()
        else:
            self.skip(ctype)

    def varint(self):
        # the header walks spend most of their time here: index the
        # buffer directly, one-byte values (the common case) first
        d = self.d
        p = self.p
        b = d[p]
        p += 1
        if b < 0x80:
            self.p = p
            return b
        out = b & 0x7F
        shift = 7
        while True:
            b = d[p]
            p += 1
            out |= (b & 0x7F) << shift
            if b < 0x80:
                self.p = p
                return out
            shift += 7

    def zigzag(self):
        v = self.varint()
        return (v >> 1) ^ -(v & 1)

    def skip(self, ctype):
        if ctype in (_CT_TRUE, _CT_FALSE):
            return
        if ctype == _CT_BYTE:
            self.byte()
        elif ctype in (_CT_I16, _CT_I32, _CT_I64):
            self.varint()
        elif ctype == _CT_DOUBLE:
            self.p += 8
        elif ctype == _CT_BINARY:
            n = self.varint()  # NB: varint() moves p; don't fold into +=
            self.p += n
        elif ctype in (_CT_LIST, _CT_SET):
            b = self.byte()
            n = b >> 4
            et = b & 0xF
            if n == 15:
                n = self.varint()
            self._need(n)  # every element is >= 1 byte
            for _ in range(n):
                self.skip_elem(et)
        elif ctype == _CT_MAP:
            n = self.varint()
            self._need(n)
            if n:
                kv = self.byte()
                for _ in range(n):
                    self.skip_elem(kv >> 4)
                    self.skip_elem(kv & 0xF)
        elif ctype == _CT_STRUCT:
            last = 0
            while True:
                b = self.byte()
                if b == _CT_STOP:
                    return
                delta = b >> 4
                ft = b & 0xF
                last = last + delta if delta else self.zigzag()
                self.skip(ft)
        else:
            raise ValueError(f"unknown thrift compact type {ctype}")

    def list_header(self) -> tuple[int, int]:
        """(count, element ctype) of a LIST/SET, count bounded by the
        bytes left (every element is >= 1 byte)."""
        b = self.byte()
        n = b >> 4
        if n == 15:
            n = self.varint()
        self._need(n)
        return n, b & 0xF

    def binary(self) -> bytes:
        n = self.varint()
        self._need(n)
        out = bytes(self.d[self.p:self.p + n])
        self.p += n
        return out

    def read_struct_fields(self):
        """Yield (field_id, ctype) and leave .p at each value start;
        caller must consume or .skip(ctype)."""
        last = 0
        d = self.d
        while True:
            b = d[self.p]
            self.p += 1
            if b == _CT_STOP:
                return
            delta = b >> 4
            ft = b & 0xF
            if delta:
                last = last + delta
            else:
                last = self.zigzag()
            yield last, ft


@dataclass
class PageInfo:
    page_type: int          # 0 data, 2 dictionary, 3 data_v2
    comp_offset: int        # absolute offset of the page payload
    comp_size: int
    uncomp_size: int
    # v2 data pages: rep+def levels are stored UNCOMPRESSED as the first
    # lvl_bytes of the payload; only the rest is codec-compressed (and
    # only when is_compressed)
    lvl_bytes: int = 0
    is_compressed: bool = True
    # first bytes of the VALUES region (payload after any v2 level
    # prefix), captured during the header walk — GZIP pages need the
    # member header parsed on CPU (RFC 1952)
    head: bytes = b""
    # what the column decode needs (csrc/parquet_decode.hip); defaults
    # keep positional construction and equality of the fields above
    num_values: int = 0     # level entries (data) / entries (dictionary)
    encoding: int = -1      # value encoding (ENC_*)
    def_encoding: int = -1  # v1 only; v2 levels are always RLE
    rep_encoding: int = -1
    rep_bytes: int = 0      # v2: byte length of the repetition levels
    def_bytes: int = 0      # v2: byte length of the definition levels
    num_nulls: int = 0      # v2
    num_rows: int = 0       # v2


PAGE_DATA = 0
PAGE_INDEX = 1
PAGE_DICTIONARY = 2
PAGE_DATA_V2 = 3

ENC_PLAIN = 0
ENC_PLAIN_DICTIONARY = 2
ENC_RLE = 3
ENC_BIT_PACKED = 4
ENC_DELTA_BINARY_PACKED = 5
ENC_DELTA_LENGTH_BYTE_ARRAY = 6
ENC_DELTA_BYTE_ARRAY = 7
ENC_RLE_DICTIONARY = 8
ENC_BYTE_STREAM_SPLIT = 9
ENCODING_NAMES = {0: "PLAIN", 2: "PLAIN_DICTIONARY", 3: "RLE",
                  4: "BIT_PACKED", 5: "DELTA_BINARY_PACKED",
                  6: "DELTA_LENGTH_BYTE_ARRAY", 7: "DELTA_BYTE_ARRAY",
                  8: "RLE_DICTIONARY", 9: "BYTE_STREAM_SPLIT"}

TYPE_BOOLEAN = 0
TYPE_INT32 = 1
TYPE_INT64 = 2
TYPE_INT96 = 3
TYPE_FLOAT = 4
TYPE_DOUBLE = 5
TYPE_BYTE_ARRAY = 6
TYPE_FIXED_LEN_BYTE_ARRAY = 7
TYPE_NAMES = {0: "BOOLEAN", 1: "INT32", 2: "INT64", 3: "INT96",
              4: "FLOAT", 5: "DOUBLE", 6: "BYTE_ARRAY",
              7: "FIXED_LEN_BYTE_ARRAY"}


def parse_page_header(data, pos: int) -> tuple[PageInfo, int]:
    """Parse one PageHeader at `pos`; returns (info, payload_offset)."""
    c = _Compact(data, pos)
    page_type = None
    comp = uncomp = None
    lvl = 0
    is_comp = True
    nvals = nnull = nrows = repb = defb = 0
    enc = denc = renc = -1

    def parse_v2(cc):
        nonlocal lvl, is_comp, nvals, nnull, nrows, enc, repb, defb
        for fid2, ft2 in cc.read_struct_fields():
            if fid2 == 1 and ft2 == _CT_I32:
                nvals = cc.zigzag()
            elif fid2 == 2 and ft2 == _CT_I32:
                nnull = cc.zigzag()
            elif fid2 == 3 and ft2 == _CT_I32:
                nrows = cc.zigzag()
            elif fid2 == 4 and ft2 == _CT_I32:
                enc = cc.zigzag()
            elif fid2 == 5:         # definition_levels_byte_length
                defb = cc.zigzag()
                lvl += defb
            elif fid2 == 6:         # repetition_levels_byte_length
                repb = cc.zigzag()
                lvl += repb
            elif fid2 == 7 and ft2 in (_CT_TRUE, _CT_FALSE):
                is_comp = ft2 == _CT_TRUE
            else:
                cc.skip(ft2)

    for fid, ft in c.read_struct_fields():
        if fid == 1 and ft in (_CT_I32, _CT_BYTE, _CT_I16):
            page_type = c.zigzag() if ft != _CT_BYTE else c.byte()
        elif fid == 2:
            uncomp = c.zigzag()
        elif fid == 3:
            comp = c.zigzag()
        elif fid == 5 and ft == _CT_STRUCT and page_type == PAGE_DATA:
            # DataPageHeader: num_values, encoding, def enc, rep enc
            for fid2, ft2 in c.read_struct_fields():
                if ft2 != _CT_I32 or fid2 > 4:
                    c.skip(ft2)
                elif fid2 == 1:
                    nvals = c.zigzag()
                elif fid2 == 2:
                    enc = c.zigzag()
                elif fid2 == 3:
                    denc = c.zigzag()
                else:
                    renc = c.zigzag()
        elif fid == 7 and ft == _CT_STRUCT and page_type == PAGE_DICTIONARY:
            # DictionaryPageHeader: num_values, encoding
            for fid2, ft2 in c.read_struct_fields():
                if ft2 != _CT_I32 or fid2 > 2:
                    c.skip(ft2)
                elif fid2 == 1:
                    nvals = c.zigzag()
                else:
                    enc = c.zigzag()
        elif fid == 8 and ft == _CT_STRUCT:
            parse_v2(c)             # DataPageHeaderV2
        else:
            c.skip(ft)
    if page_type is None or comp is None or uncomp is None:
        raise ValueError("malformed parquet PageHeader")
    if page_type != 3:
        lvl, is_comp = 0, True
        nnull = nrows = repb = defb = 0
    if nvals < 0 or nnull < 0 or nrows < 0 or repb < 0 or defb < 0:
        raise ValueError("negative count in parquet PageHeader")
    return PageInfo(page_type, c.p, comp, uncomp, lvl, is_comp, b"",
                    nvals, enc, denc, renc, repb, defb, nnull, nrows), c.p


CODEC_UNCOMPRESSED = 0
CODEC_SNAPPY = 1
CODEC_GZIP = 2
CODEC_LZ4 = 5
CODEC_ZSTD = 6
CODEC_LZ4_RAW = 7


def column_chunk_pages(data, start: int, total_compressed: int
                       ) -> list[PageInfo]:
    """Walk all pages of one column chunk (headers live in `data`, a
    buffer covering [start, start+total_compressed))."""
    pages = []
    pos = start
    end = start + total_compressed
    while pos < end:
        info, payload = parse_page_header(data, pos)
        lv = payload + info.lvl_bytes
        info.head = bytes(data[lv:lv + 64])
        pages.append(info)
        pos = payload + info.comp_size
    if pos != end:
        raise ValueError(f"column chunk walk overran: {pos} != {end}")
    return pages


@dataclass
class ChunkMeta:
    codec: int
    start: int               # first page offset (dictionary if present)
    total_compressed: int
    # for the column decode; defaults keep ChunkMeta(codec, start, total)
    path: str = ""           # dotted path_in_schema
    physical_type: int = -1  # TYPE_*
    num_values: int = 0      # level entries, nulls included
    encodings: tuple = ()    # ENC_* the writer reports for the chunk
    row_group: int = 0
    column: int = 0          # index among the row group's chunks
    num_rows: int = 0        # rows of the row group


def parse_footer(footer: bytes) -> list[ChunkMeta]:
    """Parse a parquet FileMetaData (Thrift compact) for column-chunk
    locations and codecs — self-contained, no parquet library.

    `footer` is the thrift blob (file[-8-len:-8])."""
    return parse_file_meta(footer).chunks


@dataclass
class SchemaLeaf:
    """One leaf column of the schema tree."""
    path: str                # dotted, as in ColumnMetaData.path_in_schema
    physical_type: int       # TYPE_*
    max_def: int
    max_rep: int
    # column under ONE repeated ancestor: the definition level of that
    # repeated group — an entry with def >= slot_level is a list slot
    # (an element, possibly null); 0 for a flat column
    slot_level: int = 0
    nullable: bool = False   # outermost field is OPTIONAL
    n_leaves_in_field: int = 1  # leaves under the same outermost field

    @property
    def name(self) -> str:
        """What a user calls the column: the outermost field's name when
        this is its only leaf, the dotted path otherwise."""
        return (self.path.split(".")[0] if self.n_leaves_in_field == 1
                else self.path)


@dataclass
class FileMeta:
    leaves: list             # [SchemaLeaf], in column order
    chunks: list             # [ChunkMeta], row groups in file order
    num_rows: int = 0


def _parse_schema(c: _Compact) -> list[SchemaLeaf]:
    n, et = c.list_header()
    if et != _CT_STRUCT:
        raise ValueError("FileMetaData.schema is not a struct list")
    elems = []
    for _ in range(n):
        ptype = rep = None
        name = ""
        kids = 0
        for fid, ft in c.read_struct_fields():
            if fid == 1 and ft == _CT_I32:
                ptype = c.zigzag()
            elif fid == 3 and ft == _CT_I32:
                rep = c.zigzag()
            elif fid == 4 and ft == _CT_BINARY:
                name = c.binary().decode("utf-8", "replace")
            elif fid == 5 and ft == _CT_I32:
                kids = c.zigzag()
            else:
                c.skip(ft)
        elems.append((name, ptype, rep, kids))
    leaves: list[SchemaLeaf] = []
    if not elems:
        return leaves
    pos = 1

    def walk(path, d, r, slot, top_nullable, n_kids, field_leaves):
        nonlocal pos
        for _ in range(n_kids):
            if pos >= len(elems):
                raise ValueError("schema: num_children overruns the list")
            name, ptype, rep, kids = elems[pos]
            pos += 1
            d2 = d + (rep in (1, 2))       # OPTIONAL or REPEATED
            r2 = r + (rep == 2)
            slot2 = d2 if rep == 2 else slot
            top = (rep == 1) if not path else top_nullable
            mine = [] if not path else field_leaves
            if kids > 0:
                walk(path + [name], d2, r2, slot2, top, kids, mine)
            else:
                if ptype is None:
                    raise ValueError(f"schema leaf {name!r} has no type")
                leaf = SchemaLeaf(".".join(path + [name]), ptype, d2, r2,
                                  slot2 if r2 else 0, top)
                leaves.append(leaf)
                mine.append(leaf)
            if not path:
                for lf in mine:
                    lf.n_leaves_in_field = len(mine)

    walk([], 0, 0, 0, False, max(elems[0][3], 0), [])
    return leaves


def parse_file_meta(footer: bytes) -> FileMeta:
    """FileMetaData -> schema leaves + column chunks (location, codec,
    type, path, value and row counts).  Self-contained Thrift walk."""
    chunks: list[ChunkMeta] = []
    c = _Compact(footer, 0)

    def parse_column_meta(cc: _Compact):
        codec = start = total = dict_off = data_off = None
        ptype = -1
        nvals = 0
        path = ""
        encs: tuple = ()
        for fid, ft in cc.read_struct_fields():
            if fid == 1 and ft == _CT_I32:
                ptype = cc.zigzag()
            elif fid == 2 and ft == _CT_LIST:
                n, et = cc.list_header()
                if et != _CT_I32:
                    raise ValueError("ColumnMetaData.encodings type")
                encs = tuple(cc.zigzag() for _ in range(n))
            elif fid == 3 and ft == _CT_LIST:
                n, et = cc.list_header()
                if et != _CT_BINARY:
                    raise ValueError("ColumnMetaData.path_in_schema type")
                path = ".".join(cc.binary().decode("utf-8", "replace")
                                for _ in range(n))
            elif fid == 4:
                codec = cc.zigzag()
            elif fid == 5 and ft == _CT_I64:
                nvals = cc.zigzag()
            elif fid == 7:
                total = cc.zigzag()
            elif fid == 9:
                data_off = cc.zigzag()
            elif fid == 11:
                dict_off = cc.zigzag()
            else:
                cc.skip(ft)
        start = dict_off if dict_off not in (None, 0) else data_off
        if codec is None or total is None or start is None:
            raise ValueError("incomplete ColumnMetaData")
        if nvals < 0:
            raise ValueError("negative ColumnMetaData.num_values")
        return ChunkMeta(codec, start, total, path=path,
                         physical_type=ptype, num_values=nvals,
                         encodings=encs)

    def parse_column_chunk(cc: _Compact):
        meta = None
        for fid, ft in cc.read_struct_fields():
            if fid == 3 and ft == _CT_STRUCT:
                meta = parse_column_meta(cc)
            else:
                cc.skip(ft)
        if meta is None:
            raise ValueError("ColumnChunk without meta_data")
        return meta

    def parse_row_group(cc: _Compact, rg: int):
        out = []
        rows = 0
        for fid, ft in cc.read_struct_fields():
            if fid == 1 and ft == _CT_LIST:
                n, et = cc.list_header()
                if et != _CT_STRUCT:
                    raise ValueError("RowGroup.columns type")
                for _ in range(n):
                    out.append(parse_column_chunk(cc))
            elif fid == 3 and ft == _CT_I64:
                rows = cc.zigzag()
            else:
                cc.skip(ft)
        if rows < 0:
            raise ValueError("negative RowGroup.num_rows")
        for i, cm in enumerate(out):
            cm.row_group, cm.column, cm.num_rows = rg, i, rows
        return out

    leaves: list[SchemaLeaf] = []
    num_rows = 0
    for fid, ft in c.read_struct_fields():
        if fid == 2 and ft == _CT_LIST:
            leaves = _parse_schema(c)
        elif fid == 3 and ft == _CT_I64:
            num_rows = c.zigzag()
        elif fid == 4 and ft == _CT_LIST:
            n, et = c.list_header()
            if et != _CT_STRUCT:
                raise ValueError("FileMetaData.row_groups type")
            for rg in range(n):
                chunks.extend(parse_row_group(c, rg))
        else:
            c.skip(ft)
    return FileMeta(leaves, chunks, num_rows)


def footer_span(tail8: bytes) -> int:
    """Footer thrift length from a file's last 8 bytes
    (u32 LE length + b'PAR1')."""
    import struct as _struct

    if tail8[4:] != b"PAR1":
        raise ValueError("not a parquet file (missing PAR1 trailer)")
    return _struct.unpack("<I", tail8[:4])[0]


def blob_pages(blob) -> list[tuple[int, "PageInfo"]]:
    """Page locations of a parquet blob LANDED IN HBM: footer + page
    headers are read back via small staged D2H copies (payload bytes
    never leave the device).  Returns [(codec, PageInfo)]."""
    meta, chunk_pages = blob_meta_pages(blob)
    return [(cm.codec, info)
            for cm, pages in zip(meta.chunks, chunk_pages)
            for info in pages]


def blob_meta_pages(blob) -> tuple[FileMeta, list[list["PageInfo"]]]:
    """blob_pages with the schema kept: (FileMeta, pages per column
    chunk, in meta.chunks order)."""
    import ctypes

    from ...gpu import hip

    h = hip()
    s = h.Stream(0)

    def d2h(off: int, n: int) -> bytes:
        n = min(n, blob.nbytes - off)
        out = bytearray(n)
        addr = ctypes.addressof((ctypes.c_char * n).from_buffer(out))
        h.d2h_async(addr, blob.buffer.ptr + off, n, s.handle)
        s.sync()
        return bytes(out)

    flen = footer_span(d2h(blob.nbytes - 8, 8))
    footer = d2h(blob.nbytes - 8 - flen, flen)
    meta = parse_file_meta(footer)
    out = []
    for cm in meta.chunks:
        pages = []
        # walk headers with a sliding 64 KiB host window
        pos = cm.start
        end = cm.start + cm.total_compressed
        win_off = -1
        win = b""
        while pos < end:
            if win_off < 0 or pos + 512 > win_off + len(win):
                win_off = pos
                win = d2h(pos, 64 << 10)
            info, payload = parse_page_header(win, pos - win_off)
            abs_payload = payload + win_off
            lv = payload + info.lvl_bytes
            head = bytes(win[lv:lv + 64])
            if len(head) < min(64, info.comp_size - info.lvl_bytes):
                head = d2h(abs_payload + info.lvl_bytes, 64)
            info.comp_offset, info.head = abs_payload, head
            pages.append(info)
            pos = info.comp_offset + info.comp_size
        if pos != end:
            raise ValueError("page walk overran column chunk")
        out.append(pages)
    return meta, out


def file_pages(path: str):
    """All (column-chunk codec, PageInfo) of a parquet file, using
    pyarrow only for the FOOTER metadata (offsets/codecs), never for page
    payloads.  Returns (file_bytes, [(codec, PageInfo)])."""
    import pyarrow.parquet as pq

    meta = pq.ParquetFile(path).metadata
    raw = open(path, "rb").read()
    out = []
    codec_names = {"UNCOMPRESSED": CODEC_UNCOMPRESSED,
                   "SNAPPY": CODEC_SNAPPY, "GZIP": CODEC_GZIP,
                   "ZSTD": CODEC_ZSTD,
                   # arrow writes both as raw LZ4 blocks in pages
                   "LZ4": CODEC_LZ4, "LZ4_RAW": CODEC_LZ4_RAW}
    for rg in range(meta.num_row_groups):
        for col in range(meta.num_columns):
            cc = meta.row_group(rg).column(col)
            codec = codec_names.get(cc.compression.upper())
            if codec is None:
                raise ValueError(f"unsupported codec {cc.compression}")
            start = cc.dictionary_page_offset
            if start is None or start <= 0:
                start = cc.data_page_offset
            for info in column_chunk_pages(raw, start,
                                           cc.total_compressed_size):
                out.append((codec, info))
    return raw, out


def prep_pages_gpu(blob, pages, ring=None):
    """Build the DecompressPlan for a landed parquet blob's pages: zstd
    / snappy / lz4 / raw-DEFLATE (gzip pages, member header parsed from
    PageInfo.head) kernel inputs plus (dst, src, n) device copies for
    UNCOMPRESSED pages and v2 level prefixes."""
    from ...gpu import hip
    from .compress import DecompressPlan, gzip_deflate_offset

    total = sum(p.uncomp_size for _, p in pages)
    ring = ring or hip().DeviceBuffer(max(total, 1))
    plan = DecompressPlan(ring=ring)
    streams, copies = plan.streams, plan.copies
    off = 0
    for codec, p in pages:
        lvl = p.lvl_bytes
        if lvl:
            # v2: rep+def levels pass through uncompressed
            copies.append((ring.ptr + off,
                           blob.buffer.ptr + p.comp_offset, lvl))
        src = blob.buffer.ptr + p.comp_offset + lvl
        dst = ring.ptr + off + lvl
        clen = p.comp_size - lvl
        ulen = p.uncomp_size - lvl
        if not p.is_compressed or codec == CODEC_UNCOMPRESSED:
            copies.append((dst, src, clen))
        elif codec == CODEC_ZSTD:
            streams["zstd"].append((src, clen, dst, ulen))
        elif codec == CODEC_SNAPPY:
            streams["snappy"].append((src, clen, dst, ulen))
        elif codec in (CODEC_LZ4, CODEC_LZ4_RAW):
            streams["lz4"].append((src, clen, dst, ulen))
        elif codec == CODEC_GZIP:
            gz = gzip_deflate_offset(p.head)
            # raw DEFLATE stream between the member header and the
            # 8-byte crc32+isize trailer
            streams["deflate"].append((src + gz, clen - gz - 8, dst, ulen))
        else:
            raise ValueError(f"GPU path supports ZSTD/SNAPPY/GZIP/LZ4/"
                             f"UNCOMPRESSED, got codec {codec}")
        plan.spans.append((off, p.uncomp_size))
        off += p.uncomp_size
    return plan


def launch_pages_gpu(blob, pages, ring=None):
    """Queue GPU decompression of a landed parquet blob's pages into an
    HBM ring, ASYNC on the job's own stream.  Returns (job, ring,
    spans); call job.wait() and check the results before reading the
    ring."""
    from .compress import DecompressJob

    plan = prep_pages_gpu(blob, pages, ring)
    # 16 KiB LDS window: page batches run as concurrent jobs in
    # stream_dataset, so occupancy beats far-match locality
    job = DecompressJob(plan.streams, pre_launch=plan.queue_copies,
                        window=16 << 10)
    return job, plan.ring, plan.spans


def decompress_pages_gpu(blob, pages, ring=None):
    """Synchronous wrapper around launch_pages_gpu: returns
    (ring_buffer, [(out_offset, size)]) covering every page."""
    from .compress import check_results

    job, ring, spans = launch_pages_gpu(blob, pages, ring)
    check_results(job.wait())
    return ring, spans


# ---------------------------------------------------------------------------
# Column decode: decompressed pages in HBM -> typed column tensors in HBM
# (csrc/parquet_decode.hip).  The host plans from footer + page headers
# only; the level-length prefixes, run headers and the dictionary bit
# width are read on the device.

DECODE_DESC_WORDS = 16  # u64s per PqDesc

DECODE_ERR = {0: "ok", 1: "not-run", -2: "format",
              -3: "run-overruns-num-values", -4: "stream-underrun",
              -5: "level-length", -6: "dictionary-index",
              -7: "level-out-of-range"}

_WIDTH = {TYPE_INT32: 4, TYPE_INT64: 8, TYPE_FLOAT: 4, TYPE_DOUBLE: 8}
_DICT_ENCODINGS = (ENC_PLAIN_DICTIONARY, ENC_RLE_DICTIONARY)


def raw_meta_pages(raw) -> tuple[FileMeta, list[list["PageInfo"]]]:
    """blob_meta_pages for a parquet file held in host memory."""
    flen = footer_span(bytes(raw[-8:]))
    if flen > len(raw) - 8:
        raise ValueError("parquet footer length exceeds the file")
    meta = parse_file_meta(bytes(raw[len(raw) - 8 - flen:len(raw) - 8]))
    return meta, [column_chunk_pages(raw, cm.start, cm.total_compressed)
                  for cm in meta.chunks]


@dataclass
class PagePlan:
    index: int               # position in the file's flat page list
    row_group: int
    page_no: int             # position within its column chunk
    info: PageInfo
    entry_off: int           # entries of the column before this page
    dict_index: int = -1     # flat index of the chunk's dictionary page
    dict_count: int = 0


@dataclass
class ColumnPlan:
    leaf: SchemaLeaf
    pages: list              # [PagePlan], data pages in file order
    num_entries: int         # level entries over all row groups
    num_rows: int


@dataclass
class DecodePlan:
    columns: list            # [ColumnPlan]
    skipped: dict            # column name -> why it cannot be decoded


def _leaf_unsupported(leaf: SchemaLeaf) -> str | None:
    if leaf.physical_type not in _WIDTH:
        return ("physical type "
                f"{TYPE_NAMES.get(leaf.physical_type, leaf.physical_type)}"
                " is not supported (INT32/INT64/FLOAT/DOUBLE only)")
    if leaf.max_rep > 1:
        return (f"nesting depth: max_repetition_level {leaf.max_rep} "
                "(one list level at most)")
    if leaf.max_def > 255:
        return f"max_definition_level {leaf.max_def} above 255"
    return None


def _plan_chunk(leaf, cm, pages, first_index, entry_off):
    """([PagePlan], entries) of one column chunk, or a str saying why the
    chunk cannot be decoded.  Malformed metadata raises ValueError."""
    width = _WIDTH[leaf.physical_type]
    who = f"column {leaf.name!r} row group {cm.row_group}"
    dict_index, dict_count = -1, 0
    out = []
    entries = 0
    for no, info in enumerate(pages):
        if info.page_type == PAGE_DICTIONARY:
            if no != 0:
                raise ValueError(f"{who}: dictionary page at position {no}")
            if info.encoding not in (ENC_PLAIN, ENC_PLAIN_DICTIONARY):
                return ("dictionary page encoding "
                        f"{ENCODING_NAMES.get(info.encoding, info.encoding)}")
            if info.num_values * width > info.uncomp_size:
                raise ValueError(
                    f"{who}: dictionary of {info.num_values} values "
                    f"exceeds its {info.uncomp_size}-byte page")
            dict_index, dict_count = first_index, info.num_values
            continue
        if info.page_type not in (PAGE_DATA, PAGE_DATA_V2):
            return f"page type {info.page_type}"
        if info.encoding in _DICT_ENCODINGS:
            if dict_index < 0:
                raise ValueError(f"{who} page {no}: dictionary-encoded "
                                 "without a dictionary page")
        elif info.encoding != ENC_PLAIN:
            return ("value encoding "
                    f"{ENCODING_NAMES.get(info.encoding, info.encoding)}"
                    " is not supported (PLAIN and dictionary only)")
        if info.page_type == PAGE_DATA:
            for lvl, enc, what in ((leaf.max_def, info.def_encoding,
                                    "definition"),
                                   (leaf.max_rep, info.rep_encoding,
                                    "repetition")):
                if lvl and enc == ENC_BIT_PACKED:
                    return (f"{what} levels in the deprecated BIT_PACKED "
                            "encoding")
                if lvl and enc != ENC_RLE:
                    raise ValueError(f"{who} page {no}: {what} level "
                                     f"encoding {enc}")
        elif info.rep_bytes + info.def_bytes > info.uncomp_size:
            raise ValueError(f"{who} page {no}: level bytes exceed the "
                             "page")
        out.append(PagePlan(first_index + no, cm.row_group, no, info,
                            entry_off + entries, dict_index, dict_count))
        entries += info.num_values
    if entries != cm.num_values:
        raise ValueError(f"{who}: pages hold {entries} values, the chunk "
                         f"reports {cm.num_values}")
    if leaf.max_rep == 0 and entries != cm.num_rows:
        raise ValueError(f"{who}: {entries} values for {cm.num_rows} rows")
    return out, entries


def plan_columns(meta: FileMeta, chunk_pages, columns=None) -> DecodePlan:
    """Host-only decode plan.  columns None or () selects every column
    the decoder supports and records the others in .skipped; a tuple of
    names (outermost field name, or dotted leaf path) makes an
    unsupported or unknown column a ValueError naming it."""
    leaves = meta.leaves
    ncols = len(leaves)
    if ncols == 0 or len(meta.chunks) % ncols:
        raise ValueError(f"{len(meta.chunks)} column chunks for {ncols} "
                         "schema leaves")
    for cm in meta.chunks:
        if cm.path != leaves[cm.column].path:
            raise ValueError(f"chunk path {cm.path!r} does not match "
                             f"schema leaf {leaves[cm.column].path!r}")
    explicit = bool(columns)
    if explicit:
        want = []
        for name in columns:
            hit = [i for i, lf in enumerate(leaves)
                   if name in (lf.name, lf.path)]
            if len(hit) != 1:
                raise ValueError(f"column {name!r}: not a leaf column of "
                                 f"this file ({[lf.name for lf in leaves]})")
            want.append(hit[0])
    else:
        want = list(range(ncols))
    first = []  # flat index of each chunk's first page
    at = 0
    for pages in chunk_pages:
        first.append(at)
        at += len(pages)
    plan = DecodePlan([], {})
    for ci in want:
        leaf = leaves[ci]
        why = _leaf_unsupported(leaf)
        col = ColumnPlan(leaf, [], 0, 0)
        if why is None:
            for k in range(ci, len(meta.chunks), ncols):
                cm = meta.chunks[k]
                got = _plan_chunk(leaf, cm, chunk_pages[k], first[k],
                                  col.num_entries)
                if isinstance(got, str):
                    why = got
                    break
                col.pages += got[0]
                col.num_entries += got[1]
                col.num_rows += cm.num_rows
        if why is None:
            plan.columns.append(col)
        elif explicit:
            raise ValueError(f"column {leaf.name!r}: {why}")
        else:
            plan.skipped[leaf.name] = why
    return plan


@dataclass
class Column:
    """One decoded column, tensors on the device.

    Flat column: values (int32/int64/float32/float64, one per row, null
    rows zero) and valid (bool per row; None when the column cannot hold
    nulls).  List column: values and valid are per list SLOT, offsets is
    int64 of rows + 1, list_valid is bool per row (None when the list
    field itself is not nullable)."""
    name: str
    values: object
    valid: object = None
    offsets: object = None
    list_valid: object = None


class Columns(dict):
    """name -> Column, plus .skipped (name -> reason) for the columns the
    decoder left out under columns=None."""

    def __init__(self, *a, skipped=None, **kw):
        super().__init__(*a, **kw)
        self.skipped = dict(skipped or {})


def torch_dtype(physical_type: int):
    import torch

    return {TYPE_INT32: torch.int32, TYPE_INT64: torch.int64,
            TYPE_FLOAT: torch.float32,
            TYPE_DOUBLE: torch.float64}[physical_type]


def assemble_column(leaf: SchemaLeaf, values, defs, reps,
                    num_rows: int) -> Column:
    """Entry-aligned buffers (what the kernel writes) -> Column.  Plain
    torch ops on whatever device the inputs live on; the list compaction
    synchronises."""
    import torch

    if leaf.max_rep == 0:
        valid = (defs == leaf.max_def) if leaf.max_def else None
        return Column(leaf.name, values, valid)
    slot = defs >= leaf.slot_level
    start = reps == 0
    rows = int(start.sum())
    if rows != num_rows:
        raise IOError(f"column {leaf.name!r}: repetition levels start "
                      f"{rows} rows, the footer reports {num_rows}")
    row_id = torch.cumsum(start.to(torch.int64), 0) - 1
    counts = torch.bincount(row_id[slot], minlength=rows)
    offsets = torch.zeros(rows + 1, dtype=torch.int64,
                          device=values.device)
    offsets[1:] = torch.cumsum(counts, 0)
    valid = ((defs[slot] == leaf.max_def)
             if leaf.max_def > leaf.slot_level else None)
    # the level just below the repeated group: the list exists (possibly
    # empty) at and above it
    list_valid = ((defs[start] >= leaf.slot_level - 1)
                  if leaf.slot_level > 1 else None)
    return Column(leaf.name, values[slot], valid, offsets, list_valid)


def _align16(n: int) -> int:
    return (n + 15) & ~15


class ColumnDecode:
    """Device half of one blob's DecodePlan: the entry-aligned output
    buffer, the dictionary-index scratch and one descriptor row per data
    page.  span_of(flat page index) -> (ring offset, size) locates a
    decompressed page."""

    def __init__(self, plan: DecodePlan, ring_ptr: int, span_of):
        from ...gpu import hip

        h = hip()
        self.plan = plan
        off = 0
        scr = 0
        self._layout = []
        for col in plan.columns:
            n = col.num_entries
            w = _WIDTH[col.leaf.physical_type]
            v_off, off = off, off + _align16(n * w)
            d_off = r_off = -1
            if col.leaf.max_def:
                d_off, off = off, off + _align16(n)
            if col.leaf.max_rep:
                r_off, off = off, off + _align16(n)
            self._layout.append((v_off, d_off, r_off))
            scr += sum(_align16(4 * p.info.num_values) for p in col.pages
                       if p.info.encoding in _DICT_ENCODINGS)
        self.out = h.DeviceBuffer(max(off, 1))
        self._scratch = h.DeviceBuffer(scr) if scr else None
        self.rows = []
        self.pages = []      # (ColumnPlan, PagePlan) per descriptor row
        scr = 0
        for col, (v_off, d_off, r_off) in zip(plan.columns, self._layout):
            leaf = col.leaf
            w = _WIDTH[leaf.physical_type]
            for p in col.pages:
                info = p.info
                s_off, s_len = span_of(p.index)
                is_dict = info.encoding in _DICT_ENCODINGS
                dict_ptr = 0
                if is_dict:
                    dict_ptr = ring_ptr + span_of(p.dict_index)[0]
                scratch = 0
                if is_dict:
                    scratch = self._scratch.ptr + scr
                    scr += _align16(4 * info.num_values)
                v2 = info.page_type == PAGE_DATA_V2
                params = (w | int(is_dict) << 8 | int(v2) << 16
                          | leaf.max_def << 24 | leaf.max_rep << 32)
                e = p.entry_off
                self.rows.append((
                    ring_ptr + s_off, s_len, dict_ptr, p.dict_count,
                    self.out.ptr + v_off + e * w,
                    self.out.ptr + d_off + e if d_off >= 0 else 0,
                    self.out.ptr + r_off + e if r_off >= 0 else 0,
                    scratch, info.num_values, params,
                    info.rep_bytes, info.def_bytes,
                    1, 0, 0, 0))     # status 1: the kernel has not run
                self.pages.append((col, p))

    def finish(self, results) -> Columns:
        """results: (status, non_null, consumed) per descriptor row, read
        after the stream finished.  Raises IOError naming every failed
        page's column, row group, page and status."""
        import torch

        bad = [f"column {col.leaf.name!r} row group {p.row_group} page "
               f"{p.page_no}: status {st} ({DECODE_ERR.get(st, '?')})"
               for (col, p), (st, _, _) in zip(self.pages, results)
               if st != 0]
        if bad:
            raise IOError("GPU parquet decode failed: " + "; ".join(bad[:8]))
        flat = torch.from_dlpack(self.out.to_dlpack())
        out = Columns(skipped=self.plan.skipped)
        for col, (v_off, d_off, r_off) in zip(self.plan.columns,
                                              self._layout):
            leaf = col.leaf
            n = col.num_entries
            w = _WIDTH[leaf.physical_type]
            vals = flat[v_off:v_off + n * w].view(
                torch_dtype(leaf.physical_type))
            defs = flat[d_off:d_off + n] if d_off >= 0 else None
            reps = flat[r_off:r_off + n] if r_off >= 0 else None
            if leaf.max_rep and defs is None:
                raise IOError(f"column {leaf.name!r}: repeated without "
                              "definition levels")
            out[leaf.name] = assemble_column(leaf, vals, defs, reps,
                                             col.num_rows)
        return out


class DecodeLaunch:
    """One parquet_decode launch over the descriptor rows of one or more
    ColumnDecodes.  post(stream_handle) is a DecompressJob post_launch hook:
    pinned descriptor block up, kernel, block back, all on the stream
    that decompressed the pages."""

    def __init__(self, decodes):
        self.decodes = list(decodes)
        self._n = sum(len(d.rows) for d in self.decodes)
        self._results = None

    def post(self, handle) -> None:
        import struct

        from ...gpu import hip

        if not self._n:
            return
        h = hip()
        nd = self._n * DECODE_DESC_WORDS * 8
        self._pin = h.PinnedPool(nd, 1)
        desc = self._pin.slab_view(0)
        i = 0
        for d in self.decodes:
            for row in d.rows:
                struct.pack_into("<16Q", desc, i * DECODE_DESC_WORDS * 8,
                                 *row)
                i += 1
        self._dbuf = h.DeviceBuffer(nd)
        addr = self._pin.slab_ptr(0)
        h.h2d_async(self._dbuf.ptr, addr, nd, handle)
        h.parquet_decode(self._dbuf.ptr, self._n, handle)
        h.d2h_async(addr, self._dbuf.ptr, nd, handle)

    def results(self, decode: ColumnDecode):
        """(status, non_null, consumed) rows of one ColumnDecode; call
        after the job's wait()."""
        import struct

        if self._results is None:
            raw = (bytes(self._pin.slab_view(0)[:self._n
                                                * DECODE_DESC_WORDS * 8])
                   if self._n else b"")
            res = []
            for i in range(self._n):
                st, nn, used = struct.unpack_from(
                    "<qQQ", raw, (i * DECODE_DESC_WORDS + 12) * 8)
                res.append((st, nn, used))
            self._results = res
        lo = 0
        for d in self.decodes:
            if d is decode:
                return self._results[lo:lo + len(d.rows)]
            lo += len(d.rows)
        raise KeyError("decode is not part of this launch")


class PendingColumns:
    """What launch_columns_gpu returns next to the job: finish() after
    job.wait() gives the Columns."""

    def __init__(self, decode, launch, ring):
        self.decode, self.launch, self.ring = decode, launch, ring

    def finish(self) -> Columns:
        return self.decode.finish(self.launch.results(self.decode))


def launch_columns_gpu(blob, columns=None):
    """Queue decompression of the pages the selected columns need and
    then their decode, ASYNC on the job's own stream.  Returns (job,
    pending): job.wait(), check the decompression results, then
    pending.finish()."""
    from .compress import DecompressJob

    meta, chunk_pages = blob_meta_pages(blob)
    plan = plan_columns(meta, chunk_pages, columns)   # raises before launch
    flat = [(cm.codec, info)
            for cm, pages in zip(meta.chunks, chunk_pages)
            for info in pages]
    need = sorted({i for col in plan.columns for p in col.pages
                   for i in (p.index, p.dict_index) if i >= 0})
    prep = prep_pages_gpu(blob, [flat[i] for i in need])
    where = dict(zip(need, prep.spans))
    decode = ColumnDecode(plan, prep.ring.ptr, where.__getitem__)
    launch = DecodeLaunch([decode])
    job = DecompressJob(prep.streams, pre_launch=prep.queue_copies,
                        post_launch=launch.post, window=16 << 10)
    return job, PendingColumns(decode, launch, prep.ring)


def decode_columns_gpu(blob, columns=None) -> Columns:
    """Decode columns of a parquet blob landed in HBM into typed device
    tensors: returns Columns (name -> Column, plus .skipped).

    Supported: physical types INT32, INT64, FLOAT and DOUBLE; PLAIN,
    PLAIN_DICTIONARY and RLE_DICTIONARY value encodings; v1 and v2 data
    pages; flat columns (nullable or not, also inside structs) and
    columns under one list level.  Logical types over those physical
    types (dates, times, timestamps, decimals stored in INT32/INT64,
    unsigned and narrow integers) come back as the PHYSICAL integer; the
    caller reinterprets them.

    columns=None decodes every supported column and lists the others in
    .skipped; a tuple of names makes an unsupported one a ValueError,
    raised before anything is launched.  A page the kernel rejects
    raises IOError naming column, row group, page and status."""
    from .compress import check_results

    job, pending = launch_columns_gpu(blob, columns)
    check_results(job.wait())
    return pending.finish()
