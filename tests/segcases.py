"""An independent model of gcl_tx_seg (include/gclassify.h) and the cases the
host and GPU tests share.  The model is a literal transcription of the
reference's loops -- pos, end, the do ... while, MIN(end - pos, mss), the push
test -- with the reference's line on every step; it is not the closed form the
header states and shares no code with csrc/gcl_seg.h, so the closed form is
pinned to the loop.  The layout is laid down frame by frame with Python
integers (no wrap), and the NOSPACE writes are produced as "once a write does
not fit, nothing later is sent": the suffix the header claims."""
import functools

import numpy as np

SEND_DTYPE = np.dtype([("lip", "<u4"), ("rip", "<u4"), ("lport", "<u2"), ("rport", "<u2"),
                       ("proto", "u1"), ("ecn", "u1"), ("mss", "<u2"), ("snd_nxt", "<u4"),
                       ("ack", "<u4"), ("win", "<u2"), ("pad", "<u2"), ("len", "<u4"),
                       ("winlen", "<u4"), ("pad2", "<u4"), ("src_off", "<u8")])
DESC_DTYPE = np.dtype([("lip", "<u4"), ("rip", "<u4"), ("lport", "<u2"), ("rport", "<u2"),
                       ("proto", "u1"), ("tcp_flags", "u1"), ("tcp_off", "u1"), ("ecn", "u1"),
                       ("seq", "<u4"), ("ack", "<u4"), ("win", "<u2"), ("paylen", "<u2"),
                       ("pad", "<u4")])
WRITE_DTYPE = {"status": np.uint8, "sent": np.uint32, "snd_nxt_out": np.uint32, "seg_first": np.uint32,
               "nseg": np.uint32}
SEG_DTYPE = {"desc": DESC_DTYPE, "frame_off": np.uint64, "src_off": np.uint64, "len": np.uint16,
             "dst_off": np.uint64, "send_idx": np.uint32}
OK, REFUSED, NOSPACE = 0, 1, 2
C_OK, C_REFUSED, C_NOSPACE, C_SEGS, C_BYTES, C_PUSH, C_NR = 0, 1, 2, 3, 4, 5, 8
TCP_PUSH, TCP_ACK = 0x08, 0x10     # inc/net/tcp.h
SENTINEL = 0xA5
GUARD = 37                         # entries every per-segment array has past seg_cap
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def tcp_tx_send(snd_nxt, length, mss, push=True):
    """runtime/net/tcp_out.c:313-386 with no tx_pending: the segments as
    (seg_seq, seglen, flags, pos), and the return value."""
    segs = []
    pos = 0                                        # :316  pos = buf
    end = pos + length                             # :317  end = pos + len
    while True:                                    # :329  do {
        seglen = min(end - pos, mss)               # :337  seglen = MIN(end - pos, mss)
        seg_seq = snd_nxt                          # :347  m->seg_seq = c->pcb.snd_nxt
        seg_end = snd_nxt + seglen                 # :348  m->seg_end = c->pcb.snd_nxt + seglen
        flags = TCP_ACK                            # :349  m->flags = TCP_ACK
        src = pos                                  # :354  memcpy(mbuf_put(m, seglen), pos, seglen)
        snd_nxt = (snd_nxt + seglen) & M32         # :355  store_release(&c->pcb.snd_nxt, ... + seglen)
        pos += seglen                              # :356  pos += seglen
        if push and pos == end:                    # :366  if (push && pos == end)
            flags |= TCP_PUSH                      # :367      m->flags |= TCP_PUSH
        segs.append((seg_seq, seg_end - seg_seq, flags, src))   # :368  tcp_push_tcphdr(m, c, m->flags, 5, ...)
        if not pos < end:                          # :380  } while (pos < end)
            break
    ret = 0                                        # :318
    if pos > 0:                                    # :383  if (pos - (const char *)buf > 0)
        ret = pos                                  # :384      ret = pos - (const char *)buf
    return segs, ret, snd_nxt


def write_segments(w, udp_max):
    """One write -> None (refused) or (segments, return value, snd_nxt after);
    a segment is (seq, paylen, tcp_flags, tcp_off, byte position)."""
    if w["proto"] == 6:
        if w["mss"] == 0:
            return None
        length = min(int(w["len"]), int(w["winlen"]))           # tcp.c:1374  MIN(len, winlen), push = true
        segs, ret, nxt = tcp_tx_send(int(w["snd_nxt"]), length, int(w["mss"]), True)
        return [(s, n, f, 5, p) for s, n, f, p in segs], ret, nxt
    if w["proto"] == 17:
        if int(w["len"]) > udp_max:                              # udp.c:590  if (len > udp_get_payload_size())
            return None                                          # udp.c:591      return -EMSGSIZE
        return [(0, int(w["len"]), 0, 0, 0)], int(w["len"]), (int(w["snd_nxt"]) + int(w["len"])) & M32
    return None


def blank(m, seg_cap, guard=GUARD):
    """Every output pre-filled with the sentinel, the per-segment arrays
    @guard entries longer than seg_cap."""
    out = {f: np.full(max(m, 1), SENTINEL, dtype=np.uint8).repeat(np.dtype(dt).itemsize).view(dt)
           for f, dt in WRITE_DTYPE.items()}
    for f, dt in SEG_DTYPE.items():
        out[f] = np.full((seg_cap + guard) * np.dtype(dt).itemsize, SENTINEL, dtype=np.uint8).view(dt)
    out["total_segs"] = np.full(1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    out["total_bytes"] = np.full(1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    return out


def model(case):
    send, cap = case["send"], case["seg_cap"]
    stride, lead, base, flen = case["stride"], case["lead"], case["frame_base"], case["frames_len"]
    m = len(send)
    out = blank(m, cap)
    counts = np.zeros(C_NR, dtype=np.uint64)
    S = 0            # segments of the writes so far that were not refused
    at = base        # where the next frame's slot or padded frame starts
    full = False     # a write did not fit: nothing later is sent
    g = 0            # segments written
    used = 0
    for i in range(m):
        w = send[i]
        r = write_segments(w, case["udp_max"])
        hl = 20 if w["proto"] == 6 else 8
        if r is not None and stride and max(lead + 34 + hl + s[1] for s in r[0]) > stride:
            r = None     # the largest frame does not fit a slot
        out["seg_first"][i] = min(S, cap)
        if r is None:
            out["status"][i], out["sent"][i], out["snd_nxt_out"][i], out["nseg"][i] = REFUSED, 0, w["snd_nxt"], 0
            counts[C_REFUSED] += 1
            continue
        segs, ret, nxt = r
        # lay the write's frames down one by one
        frames, pos = [], at
        for s in segs:
            frames.append(pos + lead)
            pos += stride if stride else (34 + hl + s[1] + 15) // 16 * 16
        # slots: whole slots inside frames_len; packed: the padded frames behind frame_base + lead
        end = pos if stride else pos + lead
        if not full and (S + len(segs) > cap or (flen != 0 and end > flen)):
            full = True
        S += len(segs)
        if full:
            out["status"][i], out["sent"][i], out["snd_nxt_out"][i], out["nseg"][i] = NOSPACE, 0, w["snd_nxt"], 0
            counts[C_NOSPACE] += 1
            at = pos     # the sums count the writes that did not fit too
            continue
        out["status"][i], out["sent"][i], out["snd_nxt_out"][i], out["nseg"][i] = OK, ret, nxt, len(segs)
        for (seq, n, fl, off, p), fo in zip(segs, frames):
            d = out["desc"][g]
            d["lip"], d["rip"], d["lport"], d["rport"] = w["lip"], w["rip"], w["lport"], w["rport"]
            d["proto"], d["tcp_flags"], d["tcp_off"], d["ecn"] = w["proto"], fl, off, w["ecn"]
            tcp = w["proto"] == 6
            d["seq"], d["ack"], d["win"] = seq, (w["ack"] if tcp else 0), (w["win"] if tcp else 0)
            d["paylen"], d["pad"] = n, 0
            out["frame_off"][g] = fo & M64
            out["src_off"][g] = (int(w["src_off"]) + p) & M64
            out["len"][g] = n
            out["dst_off"][g] = (fo + 14 + 20 + hl) & M64
            out["send_idx"][g] = i
            counts[C_PUSH] += 1 if fl & TCP_PUSH else 0
            g += 1
        used += pos - at
        at = pos
        counts[C_OK] += 1
        counts[C_BYTES] += ret
    counts[C_SEGS] = g
    out["total_segs"][0] = g
    out["total_bytes"][0] = used
    out["counts"] = counts
    return out


def compare(got, want, what=""):
    for f in list(WRITE_DTYPE) + list(SEG_DTYPE) + ["total_segs", "total_bytes"]:
        if got.get(f) is None:
            continue
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.shape == b.shape, (what, f, a.shape, b.shape)
        if not np.array_equal(a, b):
            bad = np.nonzero(a != b)[0][:5]
            raise AssertionError((what, f, bad.tolist(), a[bad].tolist(), b[bad].tolist()))


def run_host(g, case, send_idx=True, counts=True):
    """gcl_tx_seg_host over sentinel-filled outputs; (outputs, counts)."""
    out = blank(len(case["send"]), case["seg_cap"])
    if not send_idx:
        out["send_idx"] = None
    cnt = np.full(C_NR, 5, dtype=np.uint64) if counts else None
    g.tx_seg_host(case["send"], case["seg_cap"], stride=case["stride"], lead=case["lead"],
                  frame_base=case["frame_base"], frames_len=case["frames_len"], udp_max=case["udp_max"],
                  blocks=case.get("blocks", 0), out=out, counts=cnt)
    return out, (None if cnt is None else cnt - np.uint64(5))


# ---------------------------------------------------------------------------
# the cases

def sends(rows):
    """rows of dicts -> SEND_DTYPE; a plausible tuple where a row names none"""
    a = np.zeros(len(rows), dtype=SEND_DTYPE)
    for i, r in enumerate(rows):
        a[i]["lip"], a[i]["rip"] = 0x0A000005, 0x0A000100 + (i & 0xFF)
        a[i]["lport"], a[i]["rport"] = 4000 + (i & 0xFFF), 80 + (i % 7)
        a[i]["proto"], a[i]["mss"], a[i]["ecn"] = 6, 1460, (0x82 if i % 3 == 0 else 0)
        a[i]["snd_nxt"], a[i]["ack"], a[i]["win"] = (0x1000 * i + 7) & M32, 0x55550000 + i, 1000 + i
        a[i]["winlen"], a[i]["src_off"] = 1 << 20, 4096 * i
        for k, v in r.items():
            a[i][k] = v
    return a


def case(send, seg_cap, stride=0, lead=0, frame_base=0, frames_len=0, udp_max=1472, **kw):
    return dict(send=send, seg_cap=seg_cap, stride=stride, lead=lead, frame_base=frame_base,
                frames_len=frames_len, udp_max=udp_max, **kw)


MSS = (1, 7, 536, 1460, 65535)


def grid_rows():
    """every mss x L in {0, 1, mss - 1, mss, mss + 1, several mss}, the window
    below, at and above the length, seq wrapping 2^32, src_off near 2^64; UDP
    at and one past udp_max, empty; a bad proto; mss 0"""
    rows = []
    for mss in MSS:
        several = 3 * mss + 5 if mss > 7 else 40 * mss + 3
        for L in sorted({0, 1, mss - 1, mss, mss + 1, several}):
            for win in sorted({max(L - 1, 0), L, L + 1, L // 2, 1 << 20}):
                rows.append(dict(mss=mss, len=L, winlen=win))
    rows.append(dict(mss=536, len=5000, snd_nxt=M32 - 1000))
    rows.append(dict(mss=7, len=50, snd_nxt=M32))
    rows.append(dict(mss=1460, len=4000, src_off=M64 - 2000))
    rows.append(dict(mss=1, len=3, src_off=M64))
    for L in (0, 1, 1471, 1472, 1473, 70000):
        rows.append(dict(proto=17, len=L, winlen=0, mss=0))
    rows.append(dict(proto=1, len=10))
    rows.append(dict(proto=0, len=10))
    rows.append(dict(proto=6, mss=0, len=10))
    return rows


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case, the ones the host and the GPU both run"""
    c = {}
    rows = grid_rows()
    for lead in range(16):
        c[f"packed_lead{lead}"] = case(sends(rows), 4096, lead=lead, frame_base=64 * lead)
    for lead in (0, 1, 15):
        c[f"slots_lead{lead}"] = case(sends(rows), 4096, stride=2048, lead=lead, frame_base=4096)
    # a slot one byte too small for the full segment, and exactly big enough
    small = [dict(mss=536, len=2000), dict(mss=536, len=100), dict(proto=17, len=100, mss=0),
             dict(proto=17, len=548, mss=0), dict(proto=17, len=549, mss=0), dict(mss=537, len=2000)]
    c["slot_exact"] = case(sends(small), 64, stride=3 + 34 + 20 + 536, lead=3)
    c["slot_small"] = case(sends(small), 64, stride=3 + 34 + 20 + 536 - 1, lead=3)
    # seg_cap 0, mid-write, exactly at a write's end, ample
    caps = [dict(mss=100, len=250), dict(proto=9), dict(mss=100, len=400), dict(proto=17, len=20, mss=0),
            dict(mss=10, len=5)]
    for cap in (0, 1, 3, 5, 7, 8, 9, 64):
        c[f"cap{cap}_packed"] = case(sends(caps), cap, lead=2)
        c[f"cap{cap}_slots"] = case(sends(caps), cap, stride=256, lead=2)
    # frames_len cutting the layouts: the packed writes take 160 + 160 + 112, 4 x 160, 64 and 64 bytes
    for flen in (1, 100, 1002 + 431, 1002 + 432, 1002 + 1071, 1002 + 1072, 1002 + 1136, 1002 + 1199,
                 1002 + 1200, 5000):
        c[f"flen{flen}_packed"] = case(sends(caps), 64, lead=2, frame_base=1000, frames_len=flen)
    for flen in (1, 999, 1000 + 3 * 256 - 1, 1000 + 3 * 256, 1000 + 7 * 256, 1000 + 8 * 256, 1000 + 9 * 256 - 1, 1000 + 9 * 256):
        c[f"flen{flen}_slots"] = case(sends(caps), 64, stride=256, lead=2, frame_base=1000, frames_len=flen)
    return c


CASE_NAMES = sorted(cases())


@functools.lru_cache(maxsize=None)
def models():
    return {n: model(c) for n, c in cases().items()}


def random_case(rng, m, seg_cap=None, stride=None, refused=0.1, max_segs=6, blocks=0):
    """m plausible writes, a share of them refused, each of a few segments"""
    rows = []
    for i in range(m):
        if rng.random() < refused:
            rows.append(dict(proto=int(rng.choice([0, 1, 41])), len=int(rng.integers(0, 100))))
        elif rng.random() < 0.3:
            rows.append(dict(proto=17, mss=0, len=int(rng.integers(0, 1473)), winlen=0))
        else:
            mss = int(rng.choice([1, 7, 100, 536, 1460]))
            L = int(rng.integers(0, max_segs * mss + 1))
            rows.append(dict(mss=mss, len=L, winlen=int(rng.choice([L, L, 1 << 20, L // 2])),
                             snd_nxt=int(rng.integers(0, 1 << 32))))
    s = sends(rows)
    if stride is None:
        stride = int(rng.choice([0, 2048]))
    lead = int(rng.integers(0, 16))
    if seg_cap is None:
        seg_cap = m * max_segs + 1
    return case(s, seg_cap, stride=stride, lead=lead, frame_base=16 * int(rng.integers(0, 100)), blocks=blocks)
