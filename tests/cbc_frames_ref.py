"""Reference model of the record framing loops for the tests, in plain Python
over a pluggable per-record protect / unprotect function:

  ssl_get_next_record / mbedtls_ssl_write_record for a TLS stream
      (library/ssl_msg.c:4700-4900, :3561-3776, :3810-4017, :2648-2793), and
  their DTLS 1.2 datagram forms (fetch_input :1877-2000, the datagram rules
      :4727-4873, the anti-replay window :3248-3306, epochs, badmac_limit,
      connection IDs).

The loops know nothing about a cipher: a `Protector` seals and opens one
record.  `OracleAead` plugs in the oracle's AEAD Transform (which pins this
model against oracle/stream.c and oracle/dtls.c), `CbcProtector` the AES-CBC +
HMAC model of tests/cbc_ref.py.  Results have the shape of the oracle's
stream_* / dtls_* calls, so a test compares either with the same code.
Test-side only.
"""
from __future__ import annotations

from dataclasses import dataclass

E_BAD_INPUT_DATA = -135
E_INVALID_MAC = -0x7180
E_INVALID_RECORD = -0x7200
E_INTERNAL_ERROR = -0x6C00
E_UNEXPECTED_CID = -0x6000
E_COUNTER_WRAPPING = -0x6B80
E_UNEXPECTED_RECORD = -0x6700
E_EARLY_MESSAGE = -0x6480
E_CONN_EOF = -0x7280
DTLS_DROPPED, DTLS_NOT_REACHED = 1, 2
MSG_CID = 25
IN_CONTENT_LEN = 16384

# ssl_misc.h:283-400.  AEAD-only build: MAC_ADD 16, PADDING_ADD 0; a build with
# CBC and SHA-384 HMAC suites: MAC_ADD 48, PADDING_ADD 256.  MAX_IV_LENGTH 16,
# MAX_CID_EXPANSION 16 and CID_IN / OUT_LEN_MAX 32 in the DTLS build.
_TLS_BUF = {False: 13 + (16 + 16 + 0) + 16384, True: 13 + (16 + 48 + 256) + 16384}
_DTLS_BUF = {False: 13 + (16 + 16 + 0 + 16) + 16384 + 32, True: 13 + (16 + 48 + 256 + 16) + 16384 + 32}


@dataclass
class Limits:
    max_in_record: int        # in_buf_len less the 8-byte in_hdr offset
    out_buf_space: int        # out_buf_len - (out_iv - out_buf)
    dtls_max_datagram: int    # MBEDTLS_SSL_IN_BUFFER_LEN
    dtls_out_buffer_len: int  # MBEDTLS_SSL_OUT_BUFFER_LEN


def limits(cbc: bool) -> Limits:
    return Limits(_TLS_BUF[cbc] - 8, _TLS_BUF[cbc] - 13, _DTLS_BUF[cbc], _DTLS_BUF[cbc])


class Protector:
    """One transform direction.  head: out_msg - out_iv (explicit IV room);
    tls13; cid: out_cid when sealing, in_cid when opening; lim: the build's
    buffer limits.  seal / open return (status, data_offset, data_len, type,
    buf) as mbedtls_ssl_encrypt_buf / _decrypt_buf leave the record."""
    head = 0
    tls13 = False
    cid = b""
    lim = limits(False)

    def wire_body(self, n: int, dtls: bool) -> int:
        raise NotImplementedError

    def seal(self, buf, buf_len, data_offset, data_len, ctr, rtype, ver, k):
        raise NotImplementedError

    def open(self, buf, data_offset, data_len, ctr, rtype, ver, cid):
        raise NotImplementedError


class OracleAead(Protector):
    """The oracle's AEAD Transform (oracle.Transform), cid = its CID of the
    direction in use."""

    def __init__(self, t, head, cid=b""):
        import oracle as O
        self.O, self.t, self.head, self.cid = O, t, head, cid
        self.tls13 = t.tls_version == O.TLS1_3

    def wire_body(self, n, dtls):
        return (self.O.dtls_record_wire(self.t, n) - 13 - len(self.cid)) if dtls else \
            self.O.stream_record_wire(self.t, n) - 5

    def seal(self, buf, buf_len, data_offset, data_len, ctr, rtype, ver, k):
        rec = self.O.Record(ctr=ctr, type=rtype, ver=ver, buf=buf, data_offset=data_offset, data_len=data_len,
                            buf_len=buf_len)
        st = self.t.encrypt_buf(rec)
        return st, rec.data_offset, rec.data_len, rec.type, rec.buf

    def open(self, buf, data_offset, data_len, ctr, rtype, ver, cid):
        rec = self.O.Record(ctr=ctr, type=rtype, ver=ver, buf=buf, data_offset=data_offset, data_len=data_len,
                            cid=cid)
        st = self.t.decrypt_buf(rec)
        return st, rec.data_offset, rec.data_len, rec.type, rec.buf


class CbcProtector(Protector):
    """tests/cbc_ref.Key; ivs(k) = the explicit IV of the connection's record k
    when sealing (the engine takes it from the caller)."""
    head = 16
    lim = limits(True)

    def __init__(self, key, ivs=None):
        from tests import cbc_ref as R
        self.R, self.key, self.cid, self.ivs = R, key, key.cid, ivs

    def wire_body(self, n, dtls):
        inner = n
        if dtls and self.cid:
            inner = n + 1 + (-(n + 1)) % 16
        ml = self.R.MACLEN[self.key.mac]
        body = inner + (0 if self.key.etm else ml)
        return 16 + (body + 16) // 16 * 16 + (ml if self.key.etm else 0)

    def seal(self, buf, buf_len, data_offset, data_len, ctr, rtype, ver, k):
        buf[data_offset - 16:data_offset] = self.ivs(k)
        r = self.R.encrypt(self.key, bytes(buf[:buf_len]), data_offset, data_len, ctr, rtype, ver)
        out = bytearray(buf)
        out[:buf_len] = r.buf
        return r.status, r.data_offset, r.data_len, r.type, out

    def open(self, buf, data_offset, data_len, ctr, rtype, ver, cid):
        r = self.R.decrypt(self.key, bytes(buf), data_offset, data_len, ctr, rtype, ver, cid)
        return r.status, r.data_offset, r.data_len, r.type, bytearray(r.buf)


def _bump(ctr: bytes, lo: int):
    """cur_out_ctr / in_ctr increment over bytes [lo, 8) (:2749-2756, :3954-3963); (ctr, wrapped)"""
    v = (int.from_bytes(ctr[lo:], "big") + 1) % (1 << (8 * (8 - lo)))
    return ctr[:lo] + v.to_bytes(8 - lo, "big"), v == 0


# ---- TLS stream ----------------------------------------------------------------
def stream_decrypt(p: Protector, data: bytes, in_ctr: bytes = bytes(8), nb_zero: int = 0, max_version: int = 0x0304):
    """Returns (res dict, [(off, data_offset, data_len, type)], buffer after)."""
    buf = bytearray(data)
    res = {"status": 0, "nrec": 0, "consumed": 0, "in_ctr": bytes(in_ctr), "nb_zero": nb_zero}
    out, pos = [], 0
    while len(buf) - pos >= 5:                                         # fetch_input(5)
        rtype, ver, dlen = buf[pos], bytes(buf[pos + 1:pos + 3]), int.from_bytes(buf[pos + 3:pos + 5], "big")
        if rtype not in (20, 21, 22, 23) or int.from_bytes(ver, "big") > max_version or dlen == 0:
            res["status"] = E_INVALID_RECORD                           # :3529-3539, :3723-3726
            break
        if 5 + dlen > p.lim.max_in_record:                             # fetch_input(rec.buf_len)
            res["status"] = E_BAD_INPUT_DATA
            break
        if len(buf) - pos < 5 + dlen:                                  # incomplete record: wait
            break
        doff, dl, typ = 5, dlen, rtype
        if not (p.tls13 and rtype == 20):                              # TLS 1.3 CCS passes undecrypted
            st, doff, dl, typ, rb = p.open(bytearray(buf[pos:pos + 5 + dlen]), 5, dlen, res["in_ctr"], rtype, ver, b"")
            buf[pos:pos + 5 + dlen] = rb
            if st:
                res["status"] = st
                break
            if typ not in (20, 21, 22, 23):                            # :3914-3917
                res["status"] = E_INVALID_RECORD
                break
            if dl == 0:                                                # :3888-3906
                if not p.tls13 and typ != 23:
                    res["status"] = E_INVALID_RECORD
                    break
                res["nb_zero"] += 1
                if res["nb_zero"] > 3:
                    res["status"] = E_INVALID_MAC
                    break
            else:
                res["nb_zero"] = 0
            res["in_ctr"], wrapped = _bump(res["in_ctr"], 0)
            if wrapped:
                res["status"] = E_COUNTER_WRAPPING
                break
        if dl > IN_CONTENT_LEN:                                        # :4011-4014
            res["status"] = E_INVALID_RECORD
            break
        out.append((pos, doff, dl, typ))
        res["nrec"] += 1
        pos += 5 + dlen
        res["consumed"] = pos
    return res, out, bytes(buf)


def _send(p: Protector, pt: bytes, rtype: int, out_ctr: bytes, max_frag: int, dtls: bool):
    """mbedtls_ssl_write until every byte is sent, one record per call;
    returns (status, wire, records, out_ctr after, [(wire offset of rec.buf, data_len)])"""
    if dtls and p.tls13:
        return E_BAD_INPUT_DATA, b"", 0, bytes(out_ctr), []
    ctr, wire, nrec, recs, off = bytes(out_ctr), bytearray(), 0, [], 0
    hdr = 13 + len(p.cid) if dtls else 5
    ver = b"\xfe\xfd" if dtls else b"\x03\x03"                         # mbedtls_ssl_write_version (:2669-2674)
    buf_len = p.lim.dtls_out_buffer_len - hdr if dtls else p.lim.out_buf_space
    while off < len(pt):
        n = min(len(pt) - off, max_frag)
        tmp = bytearray(buf_len)
        tmp[p.head:p.head + n] = pt[off:off + n]
        st, doff, dl, typ, rb = p.seal(tmp, buf_len, p.head, n, ctr, rtype, ver, nrec)
        if st:
            return st, bytes(wire), nrec, ctr, recs
        if doff != 0:                                                  # :2704-2707
            return E_INTERNAL_ERROR, bytes(wire), nrec, ctr, recs
        if dtls:
            wire += bytes([typ]) + ver + ctr + p.cid + dl.to_bytes(2, "big")
        else:
            wire += bytes([typ]) + ver + dl.to_bytes(2, "big")
        recs.append((len(wire), dl))
        wire += rb[:dl]
        off += n
        nrec += 1
        ctr, wrapped = _bump(ctr, 2 if dtls else 0)
        if wrapped:
            return E_COUNTER_WRAPPING, bytes(wire), nrec, ctr, recs
    return 0, bytes(wire), nrec, ctr, recs


def stream_encrypt(p: Protector, pt: bytes, rtype: int = 23, out_ctr: bytes = bytes(8), max_frag: int = 16384):
    """Returns (status, record stream bytes, records, out_ctr after)."""
    return _send(p, pt, rtype, out_ctr, max_frag, False)[:4]


def dtls_encrypt(p: Protector, pt: bytes, rtype: int = 23, out_ctr: bytes = bytes(8), max_frag: int = 16384):
    """Returns (status, datagrams back to back, records, out_ctr after)."""
    return _send(p, pt, rtype, out_ctr, max_frag, True)[:4]


def send_records(p, pt, rtype, out_ctr, max_frag, dtls):
    """the records of _send: [(offset of rec.buf in the wire bytes, protected length)]"""
    return _send(p, pt, rtype, out_ctr, max_frag, dtls)[4]


def out_size(p: Protector, in_len: int, max_frag: int, dtls: bool) -> int:
    """wire bytes of in_len application bytes (max_frag 0 = 16384)"""
    f = max_frag or 16384
    hdr = 13 + len(p.cid) if dtls else 5
    return sum(hdr + p.wire_body(min(f, in_len - o), dtls) for o in range(0, in_len, f))


# ---- DTLS 1.2 ------------------------------------------------------------------
@dataclass
class DtlsState:
    """The mbedtls_ssl_context / config fields of the DTLS read loop."""
    window_top: int = 0
    window: int = 0
    badmac_seen: int = 0
    badmac_limit: int = 0
    in_epoch: int = 0
    cid_len: int = 0
    anti_replay: int = 1
    ignore_unexpected_cid: int = 0
    nb_zero: int = 0


def replay_check(st: DtlsState, ctr: bytes) -> int:
    """mbedtls_ssl_dtls_replay_check (:3248-3271), 0 = acceptable"""
    seq = int.from_bytes(ctr[2:], "big")
    if not st.anti_replay or seq > st.window_top:
        return 0
    bit = st.window_top - seq
    return -1 if bit >= 64 or (st.window >> bit) & 1 else 0


def replay_update(st: DtlsState, ctr: bytes) -> None:
    """mbedtls_ssl_dtls_replay_update (:3277-3306)"""
    seq = int.from_bytes(ctr[2:], "big")
    if not st.anti_replay:
        return
    if seq > st.window_top:
        shift = seq - st.window_top
        st.window = 1 if shift >= 64 else ((st.window << shift) | 1) & ((1 << 64) - 1)
        st.window_top = seq
    elif st.window_top - seq < 64:
        st.window |= 1 << (st.window_top - seq)


def _read_version_dtls(v: bytes) -> int:
    """mbedtls_ssl_read_version, datagram transport (:6215-6228)"""
    w = int.from_bytes(v, "big")
    return ~(w - (0x0202 if w == 0xfeff else 0x0201)) & 0xffff


def _parse_header(st: DtlsState, b, rem: int):
    """the checks of ssl_parse_record_header that decide where a record ends
    (:3591-3753); None on a header error, else (type, ver, ctr, cid, data_offset, data_len)"""
    lo = 11
    if rem < lo + 2:
        return None
    rtype, cid = b[0], b""
    if st.cid_len != 0 and rtype == MSG_CID:                           # :3616-3649
        lo += st.cid_len
        if rem < lo + 2:
            return None
        cid = bytes(b[11:11 + st.cid_len])
    elif rtype < 20 or rtype > 23:
        return None
    if _read_version_dtls(bytes(b[1:3])) > 0x0303:                     # max_tls_version, ssl_tls.c:5514-5517
        return None
    dlen = int.from_bytes(b[lo:lo + 2], "big")
    if dlen == 0 or rem < lo + 2 + dlen:                               # :3723-3726, :3745-3753
        return None
    return rtype, bytes(b[1:3]), bytes(b[3:11]), cid, lo + 2, dlen


def dtls_decrypt(p: Protector, st: DtlsState, datagrams):
    """One connection's datagrams in arrival order; st is updated in place.
    Returns (res dict, [(dgram, off, data_offset, data_len, disp, type)],
    [datagram bytes after])."""
    res = {"status": E_BAD_INPUT_DATA if p.tls13 else 0, "nrec": 0, "naccepted": 0, "dgrams_done": 0,
           "invalid_dgrams": 0}
    out, after = [], []

    def list_rest(b, pos, length, d, disp):
        while length - pos >= 13:
            h = _parse_header(st, b[pos:], length - pos)
            if h is None:
                break
            out.append((d, pos, h[4], h[5], disp, h[0]))
            pos += h[4] + h[5]

    for d, dg in enumerate(datagrams):
        b = bytearray(dg)
        length = min(len(b), p.lim.dtls_max_datagram)                  # f_recv into the in buffer
        if res["status"]:
            list_rest(b, 0, length, d, DTLS_NOT_REACHED)
            after.append(bytes(b))
            continue
        if length == 0:                                                # :1968-1970
            res["status"] = E_CONN_EOF
            after.append(bytes(b))
            continue
        pos = 0
        while pos < length:
            if length - pos < 13:
                if pos == 0:
                    res["invalid_dgrams"] += 1
                else:
                    res["status"] = E_INTERNAL_ERROR                   # :1921-1926
                break
            h = _parse_header(st, b[pos:], length - pos)
            if h is None:                                              # drop the rest of the datagram
                res["invalid_dgrams"] += 1
                break
            rtype, ver, ctr, cid, doff, dlen = h
            here = pos
            pos += doff + dlen
            epoch = int.from_bytes(ctr[:2], "big")
            if epoch != st.in_epoch:                                   # :3755-3768
                out.append((d, here, doff, dlen, E_EARLY_MESSAGE if epoch == st.in_epoch + 1 else E_UNEXPECTED_RECORD,
                            rtype))
                continue
            if replay_check(st, ctr) != 0:                             # :3769-3776
                out.append((d, here, doff, dlen, E_UNEXPECTED_RECORD, rtype))
                continue
            r, o2, l2, t2, rb = p.open(bytearray(b[here:pos]), doff, dlen, ctr, rtype, ver, cid)
            b[here:pos] = rb
            if r == E_UNEXPECTED_CID and st.ignore_unexpected_cid:     # :3872-3879
                out.append((d, here, o2, l2, r, t2))
                continue
            if r == 0:
                if t2 < 20 or t2 > 23:                                 # :3914-3917
                    r = E_INVALID_RECORD
                elif l2 == 0:                                          # :3920-3941
                    if t2 != 23:
                        r = E_INVALID_RECORD
                    else:
                        st.nb_zero += 1
                        if st.nb_zero > 3:
                            r = E_INVALID_MAC
                else:
                    st.nb_zero = 0
            if r == 0:
                replay_update(st, ctr)                                 # :4003-4007
                if l2 > IN_CONTENT_LEN:
                    r = E_INVALID_RECORD
            out.append((d, here, o2, l2, r, t2))
            if r == E_INVALID_MAC:                                     # :4837-4873
                st.badmac_seen += 1 if st.badmac_limit != 0 else 0
                if st.badmac_limit != 0 and st.badmac_seen >= st.badmac_limit:
                    res["status"] = r
                else:
                    list_rest(b, pos, length, d, DTLS_DROPPED)
                break
            if r != 0:
                res["status"] = r
                break
            res["naccepted"] += 1
        if res["status"]:
            list_rest(b, pos, length, d, DTLS_NOT_REACHED)
        else:
            res["dgrams_done"] = d + 1
        after.append(bytes(b))
    res["nrec"] = len(out)
    return res, out, after
