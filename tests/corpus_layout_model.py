"""A numpy model of a resident corpus' device arrays, for the layout tests of a corpus that grows (test_gpu_corpus_append.py) and pinned
on the CPU by test_corpus_append_abi.py.

  canonical(haystacks)         the padded-16 bytes (+ the 96-byte zero tail) and the end offsets inside them
  build_view(haystacks)        the filter's view of the list as DESIGN.md section 2 describes it (one of the valid ones: the order of
                               equal-length haystacks inside a tile is free - on the device their ranks come from an LDS atomicAdd)
  check_view(haystacks, view)  decodes a view - whoever built it - back into the haystacks and checks its invariants; raises ViewError

A view: dict of vbytes (u8), vgofs (u32), vgnv (u8), vlen (u16), vperm (u16), vlong (u32).  Tiles hold 1024 haystacks, groups 64 sorted ones.
Sort key of a haystack: its length, 0 for an OUTLIER (beyond 256 bytes: not in the view, vlen 0xFFFF, listed in vlong)."""
import numpy as np

TILE, GROUP, OUTLIER_BEYOND, TAIL = 1024, 64, 256, 96


class ViewError(AssertionError):
    pass


def _b(h):
    return h if isinstance(h, (bytes, bytearray)) else h.encode("utf-8")


def canonical(haystacks):
    """(u8 bytes of the padded-16 layout + 96 zero bytes, u32 exclusive end offsets inside it)"""
    hs = [_b(h) for h in haystacks]
    ends = np.zeros(len(hs), np.uint32)
    pos = 0
    parts = []
    for i, h in enumerate(hs):
        ends[i] = pos + len(h)
        padded = (len(h) + 15) & ~15
        parts.append(bytes(h) + b"\0" * (padded - len(h)))
        pos += padded
    return np.frombuffer(b"".join(parts) + b"\0" * TAIL, np.uint8).copy(), ends


def wants_view(haystacks):
    """the criteria of the upload: not uniform, something within 256 bytes beyond 32, outliers <= n/256 + 64"""
    lens = [len(_b(h)) for h in haystacks]
    n = len(lens)
    if not n:
        return False
    uniform = min(lens) == max(lens) and max(lens) > 0
    short = [x for x in lens if x <= OUTLIER_BEYOND]
    return (not uniform) and bool(short) and max(short) > 32 and sum(x > OUTLIER_BEYOND for x in lens) <= n // 256 + 64


def _key(length):
    return 0 if length > OUTLIER_BEYOND else length


def group_code(len0):
    """(vgnv code, 16-byte units of the block) of a group whose first - longest - member has len0 bytes (0: an outlier, empty, or no member)"""
    nv = (len0 + 15) >> 4
    if not nv:
        return 0, 0
    tw = (len0 - 16 * (nv - 1) + 3) & ~3
    return nv | ((tw // 4 - 1) << 5), (nv - 1) * 64 + tw * 4


def _place(vbytes, gofs, code, slot, h):
    """writes member `slot` (0..63) of a group into its block"""
    gnv, gtw = code & 31, ((code >> 5) + 1) * 4
    base = gofs * 16
    for v in range((len(h) + 15) >> 4):
        chunk = bytes(h[16 * v:16 * v + 16]).ljust(16, b"\0")
        if v + 1 < gnv:
            at = base + v * 1024 + slot * 16
            vbytes[at:at + 16] = np.frombuffer(chunk, np.uint8)
        else:
            at = base + (gnv - 1) * 1024 + slot * gtw
            vbytes[at:at + gtw] = np.frombuffer(chunk[:gtw], np.uint8)


def build_view(haystacks, rng=None):
    """A valid view of the list.  rng: shuffles the order of equal keys inside a tile (what the device is free to do)."""
    hs = [_b(h) for h in haystacks]
    n = len(hs)
    ntiles = (n + TILE - 1) // TILE
    vperm, vlen = np.zeros(n, np.uint16), np.zeros(n, np.uint16)
    vgnv, vgofs = np.zeros(ntiles * 16, np.uint8), np.zeros(ntiles * 16, np.uint32)
    vlong = [i for i, h in enumerate(hs) if len(h) > OUTLIER_BEYOND]
    units = 0
    for t in range(ntiles):
        i0, nt = t * TILE, min(TILE, n - t * TILE)
        order = list(range(nt))
        if rng is not None:
            rng.shuffle(order)
        order.sort(key=lambda j: -_key(len(hs[i0 + j])))  # (stable)
        for p, j in enumerate(order):
            vperm[i0 + p] = j
            vlen[i0 + p] = 0xFFFF if len(hs[i0 + j]) > OUTLIER_BEYOND else len(hs[i0 + j])
        for g in range(16):
            len0 = _key(len(hs[i0 + order[g * 64]])) if g * 64 < nt else 0
            code, u = group_code(len0)
            vgnv[t * 16 + g], vgofs[t * 16 + g] = code, units
            units += u
    vbytes = np.zeros(units * 16, np.uint8)
    for t in range(ntiles):
        i0, nt = t * TILE, min(TILE, n - t * TILE)
        for p in range(nt):
            h = hs[i0 + int(vperm[i0 + p])]
            if len(h) <= OUTLIER_BEYOND:
                _place(vbytes, int(vgofs[t * 16 + p // 64]), int(vgnv[t * 16 + p // 64]), p % 64, h)
    return dict(vbytes=vbytes, vgofs=vgofs, vgnv=vgnv, vlen=vlen, vperm=vperm, vlong=np.array(vlong, np.uint32))


def check_view(haystacks, view):
    """Decodes `view` and checks it against the list; returns the decoded haystacks (None for an outlier)."""
    hs = [_b(h) for h in haystacks]
    n = len(hs)
    ntiles = (n + TILE - 1) // TILE
    vbytes, vgofs, vgnv, vlen, vperm, vlong = (np.asarray(view[k]) for k in ("vbytes", "vgofs", "vgnv", "vlen", "vperm", "vlong"))

    def need(cond, *what):
        if not cond:
            raise ViewError(" ".join(str(w) for w in what))

    need(len(vperm) == n and len(vlen) == n, "vperm / vlen hold", len(vperm), len(vlen), "entries for", n, "haystacks")
    need(len(vgnv) == ntiles * 16 and len(vgofs) == ntiles * 16, "vgnv / vgofs hold", len(vgnv), len(vgofs), "groups for", ntiles, "tiles")
    need(len(vbytes) % 16 == 0, "vbytes is not a whole number of vectors")
    outliers = sorted(i for i, h in enumerate(hs) if len(h) > OUTLIER_BEYOND)
    need(sorted(int(x) for x in vlong) == outliers, "outliers listed", sorted(int(x) for x in vlong), "expected exactly once each", outliers)
    decoded = [None] * n
    covered = np.zeros(len(vbytes), bool)
    units = 0
    for t in range(ntiles):
        i0, nt = t * TILE, min(TILE, n - t * TILE)
        perm = vperm[i0:i0 + nt].astype(np.int64)
        need(sorted(perm.tolist()) == list(range(nt)), "tile", t, ": vperm is not a permutation of its", nt, "haystacks")
        keys = [_key(len(hs[i0 + j])) for j in perm]
        need(all(keys[p] >= keys[p + 1] for p in range(nt - 1)), "tile", t, ": lengths do not descend")
        for p in range(nt):
            length = len(hs[i0 + perm[p]])
            need(int(vlen[i0 + p]) == (0xFFFF if length > OUTLIER_BEYOND else length), "tile", t, "position", p, ": vlen", int(vlen[i0 + p]), "for a haystack of", length)
        for g in range(16):
            code, u = group_code(keys[g * 64] if g * 64 < nt else 0)
            need(int(vgnv[t * 16 + g]) == code, "tile", t, "group", g, ": code", int(vgnv[t * 16 + g]), "expected", code)
            need(int(vgofs[t * 16 + g]) == units, "tile", t, "group", g, ": block at", int(vgofs[t * 16 + g]), "expected", units)
            gnv, gtw = code & 31, ((code >> 5) + 1) * 4
            base = units * 16
            units += u
            need(units * 16 <= len(vbytes), "tile", t, "group", g, ": block beyond vbytes")
            for p in range(g * 64, min(g * 64 + 64, nt)):
                h = hs[i0 + perm[p]]
                if len(h) > OUTLIER_BEYOND:
                    continue
                got = b""
                for v in range((len(h) + 15) >> 4):
                    need(v < gnv, "tile", t, "position", p, ": longer than its group")
                    at, w = (base + v * 1024 + (p % 64) * 16, 16) if v + 1 < gnv else (base + (gnv - 1) * 1024 + (p % 64) * gtw, gtw)
                    got += vbytes[at:at + w].tobytes().ljust(16, b"\0")
                    covered[at:at + w] = True
                need(got[:len(h)] == bytes(h) and not any(got[len(h):]), "tile", t, "position", p, ": decodes to", got[:64], "expected", bytes(h)[:64])
                decoded[i0 + perm[p]] = got[:len(h)]
    need(units * 16 == len(vbytes), "vbytes holds", len(vbytes), "bytes, the groups take", units * 16)
    need(not vbytes[~covered].any(), "non-zero bytes behind a group's shorter members")
    return decoded
