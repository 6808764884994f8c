"""Helpers that lay out record batches in a device arena, run them through
libtlsrec (GPU) and through the oracle (CPU), and compare.  Test-side only."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import pytest

import mbedtls_amd as M
import oracle as O
from tests.prng import prng_bytes

CIPHERS = {"AES-128-GCM": M.CIPHER_AES_128_GCM, "AES-256-GCM": M.CIPHER_AES_256_GCM,
           "CHACHA20-POLY1305": M.CIPHER_CHACHA20_POLY1305, "AES-192-GCM": M.CIPHER_AES_192_GCM,
           "AES-128-CCM": M.CIPHER_AES_128_CCM, "AES-192-CCM": M.CIPHER_AES_192_CCM,
           "AES-256-CCM": M.CIPHER_AES_256_CCM, "AES-128-CCM-8": M.CIPHER_AES_128_CCM_8,
           "AES-192-CCM-8": M.CIPHER_AES_192_CCM_8, "AES-256-CCM-8": M.CIPHER_AES_256_CCM_8,
           "ARIA-128-GCM": M.CIPHER_ARIA_128_GCM, "ARIA-192-GCM": M.CIPHER_ARIA_192_GCM,
           "ARIA-256-GCM": M.CIPHER_ARIA_256_GCM, "ARIA-128-CCM": M.CIPHER_ARIA_128_CCM,
           "ARIA-192-CCM": M.CIPHER_ARIA_192_CCM, "ARIA-256-CCM": M.CIPHER_ARIA_256_CCM,
           "CAMELLIA-128-GCM": M.CIPHER_CAMELLIA_128_GCM, "CAMELLIA-192-GCM": M.CIPHER_CAMELLIA_192_GCM,
           "CAMELLIA-256-GCM": M.CIPHER_CAMELLIA_256_GCM, "CAMELLIA-128-CCM": M.CIPHER_CAMELLIA_128_CCM,
           "CAMELLIA-192-CCM": M.CIPHER_CAMELLIA_192_CCM, "CAMELLIA-256-CCM": M.CIPHER_CAMELLIA_256_CCM}
VERSIONS = {"TLS1.2": M.VERSION_TLS1_2, "TLS1.3": M.VERSION_TLS1_3}


def keylen(cipher):
    return M.KEYLEN[cipher]


def explicit(cipher, ver):
    return ver == M.VERSION_TLS1_2 and cipher != M.CIPHER_CHACHA20_POLY1305


@dataclass
class Rec:
    slot: int
    buf: bytearray          # the whole record buffer (rec->buf .. rec->buf + buf_len)
    data_offset: int
    data_len: int
    ctr: bytes
    type: int
    ver: bytes = b"\x03\x03"
    cid: bytes = b""        # decrypt: the record's DTLS connection ID


class Batch:
    def __init__(self, slots, recs, align=16, cids=None):
        """slots: list of (cipher, version, key, iv, granularity); cids: optional
        {slot: connection ID} (the slot's out_cid / in_cid)"""
        self.slots = slots
        self.recs = recs
        self.cids = cids or {}
        offs, pos = [], 0
        for r in recs:
            offs.append(pos)
            # the record's CID bytes (decrypt) sit after its buffer
            pos += (len(r.buf) + len(r.cid) + align - 1) // align * align + align
        self.offs = offs
        self.arena = np.zeros(max(pos, 16), dtype=np.uint8)
        for r, o in zip(recs, offs):
            self.arena[o:o + len(r.buf)] = np.frombuffer(bytes(r.buf), dtype=np.uint8)
            if r.cid:
                self.arena[o + len(r.buf):o + len(r.buf) + len(r.cid)] = np.frombuffer(r.cid, dtype=np.uint8)
        d = M.records(len(recs))
        for i, (r, o) in enumerate(zip(recs, offs)):
            d[i]["buf_off"] = o
            d[i]["buf_len"] = len(r.buf)
            d[i]["data_offset"] = r.data_offset
            d[i]["data_len"] = r.data_len
            d[i]["slot"] = r.slot
            d[i]["ctr"] = np.frombuffer(r.ctr, dtype=np.uint8)
            d[i]["type"] = r.type
            d[i]["ver"] = np.frombuffer(r.ver, dtype=np.uint8)
            d[i]["cid_len"] = len(r.cid)
            d[i]["cid_off"] = len(r.buf)
        self.desc = d

    def key_materials(self):
        km = np.concatenate([M.key_material(c, v, k, iv, g) for (c, v, k, iv, g) in self.slots])
        return km

    def run_gpu(self, decrypt: bool, lanes=0, inplace=True, kt=None, mean_bytes=0, stream=None):
        """kt: an already loaded key table (e.g. filled by keytab_derive);
        mean_bytes: the record-size hint of tlsrec_batch_*_sized; stream: a
        HIP stream handle other than torch's (e.g. 2 = hipStreamPerThread)."""
        import torch
        dev = torch.device("cuda")
        own = kt is None
        if own:
            kt = M.KeyTable(max(1, len(self.slots)))
            kt.load(self.key_materials())
            for slot, cid in self.cids.items():
                kt.set_cid(slot, cid)
        arena = torch.from_numpy(self.arena.copy()).to(dev)
        out = arena if inplace else torch.zeros_like(arena)
        recs = torch.from_numpy(self.desc.view(np.uint8).copy()).to(dev)
        res = torch.zeros(len(self.recs) * 16, dtype=torch.uint8, device=dev)
        fn = M.batch_decrypt if decrypt else M.batch_encrypt
        if stream is not None:
            torch.cuda.synchronize()      # torch's fills above ran on its own stream
        fn(kt, recs, res, len(self.recs), arena, out, lanes=lanes, mean_bytes=mean_bytes, stream=stream)
        torch.cuda.synchronize()
        out_np = out.cpu().numpy()
        res_np = res.cpu().numpy().view(M.BATCH_RES)
        if own:
            kt.close()
        return out_np, res_np

    def run_oracle(self, decrypt: bool):
        outs, stats = [], []
        ts = {}
        for r in self.recs:
            c, v, k, iv, g = self.slots[r.slot]
            if r.slot not in ts:
                ts[r.slot] = O.Transform(v, c, k, k, iv, iv, granularity=g or 16)
                if r.slot in self.cids:
                    ts[r.slot].set_cid(self.cids[r.slot], self.cids[r.slot])
            t = ts[r.slot]
            rec = O.Record(ctr=r.ctr, type=r.type, ver=r.ver, buf=bytearray(r.buf),
                           data_offset=r.data_offset, data_len=r.data_len, cid=r.cid if decrypt else b"")
            st = t.decrypt_buf(rec) if decrypt else t.encrypt_buf(rec)
            outs.append(rec)
            stats.append(st)
        return outs, stats

    def compare(self, decrypt: bool, gpu_out, gpu_res, inplace=True):
        """Return list of mismatch descriptions (empty = bit-exact)."""
        o_recs, o_stats = self.run_oracle(decrypt)
        bad = []
        for i, (r, orec, ost) in enumerate(zip(self.recs, o_recs, o_stats)):
            g = gpu_res[i]
            fields = (int(g["status"]), int(g["data_offset"]), int(g["data_len"]), int(g["type"]),
                      int(g["cid_len"]) if not decrypt else 0)
            want = (ost, orec.data_offset, orec.data_len, orec.type, len(orec.cid) if not decrypt else 0)
            if fields != want:
                bad.append(f"rec {i}: fields {fields} != oracle {want}")
                continue
            o = self.offs[i]
            gbuf = bytes(gpu_out[o:o + len(r.buf)])
            if inplace:
                if gbuf != bytes(orec.buf):
                    diff = next(j for j in range(len(gbuf)) if gbuf[j] != orec.buf[j])
                    bad.append(f"rec {i}: buffer differs from byte {diff} (len {len(gbuf)})")
            elif ost == 0:
                lo, hi = orec.data_offset, orec.data_offset + orec.data_len
                if gbuf[lo:hi] != bytes(orec.buf[lo:hi]):
                    bad.append(f"rec {i}: output region differs")
        return bad


def random_slots(rng_seed, ciphers, versions, count):
    slots = []
    for i in range(count):
        c = ciphers[i % len(ciphers)]
        v = versions[(i // len(ciphers)) % len(versions)]
        b = prng_bytes(rng_seed * 1000 + i, 48)
        slots.append((c, v, b[:keylen(c)], b[32:48], 0))
    return slots


def plaintext_records(slots, lengths, seed, head=8, tail=40):
    recs = []
    for i, L in enumerate(lengths):
        s = i % len(slots)
        payload = prng_bytes(seed + i, L)
        buf = bytearray(head + L + tail)
        buf[head:head + L] = payload
        ctr = int(prng_bytes(seed ^ (i + 77), 8).hex(), 16).to_bytes(8, "big")
        recs.append(Rec(slot=s, buf=buf, data_offset=head, data_len=L, ctr=ctr,
                        type=23 if i % 5 else 22))
    return recs


def sealed_records(slots, lengths, seed, head=8, tail=40):
    """Records encrypted by the oracle, ready for a decrypt batch."""
    pre = plaintext_records(slots, lengths, seed, head, tail)
    b = Batch(slots, pre)
    outs, stats = b.run_oracle(False)
    recs = []
    for r, o, st in zip(pre, outs, stats):
        assert st == 0
        recs.append(Rec(slot=r.slot, buf=bytearray(o.buf), data_offset=o.data_offset,
                        data_len=o.data_len, ctr=r.ctr, type=o.type, ver=r.ver))
    return recs, pre


def gcm_sealed_records(slots, lengths, seed, head=8, tail=40):
    """GCM records sealed with the oracle's raw AEAD (no OUT_CONTENT_LEN cap,
    unlike the record-layer encrypt), framed as ssl_msg.c frames them:
    TLS 1.2 explicit nonce = ctr, AAD = ctr|type|ver|len16(plaintext);
    TLS 1.3 nonce = iv ^ (0^4|ctr), AAD = 23|ver|len16(ct+tag), inner type byte.
    Used for records the encrypt side may not produce (counters past 2^16)."""
    recs = []
    for i, L in enumerate(lengths):
        s = i % len(slots)
        c, v, k, iv, _ = slots[s]
        payload = prng_bytes(seed + i, L)
        ctr = int(prng_bytes(seed ^ (i + 77), 8).hex(), 16).to_bytes(8, "big")
        rtype = 23 if i % 5 else 22
        if v == M.VERSION_TLS1_3:
            inner = payload + bytes([rtype])
            nonce = bytes(a ^ b for a, b in zip(iv[:12], bytes(4) + ctr))
            aad = bytes([23]) + b"\x03\x03" + ((len(inner) + 16) & 0xffff).to_bytes(2, "big")
            ct, tag = O.gcm_encrypt(k, nonce, aad, inner)
            body = ct + tag
            wire_type = 23
        else:
            nonce = iv[:4] + ctr
            aad = ctr + bytes([rtype]) + b"\x03\x03" + (L & 0xffff).to_bytes(2, "big")
            ct, tag = O.gcm_encrypt(k, nonce, aad, payload)
            body = ctr + ct + tag
            wire_type = rtype
        buf = bytearray(head + len(body) + tail)
        buf[head:head + len(body)] = body
        recs.append(Rec(slot=s, buf=buf, data_offset=head, data_len=len(body), ctr=ctr, type=wire_type))
    return recs


# ---- the dispatchers' launch log (test-hooks build) ---------------------------
@pytest.fixture
def launch_log():
    """Route the bindings to the test-hooks library (create key tables inside
    the test), forget its launch log, and yield a reader: launch_log() ->
    [(kind, p0, p1, p2, p3)] since the reset (or the last launch_log.reset()),
    kinds as mbedtls_amd._abi.LOG_*."""
    from mbedtls_amd import _abi
    with _abi.use_library():
        _abi.launch_log_reset()

        def read(kind=None):
            log = _abi.launch_log_read()
            return [e for e in log if kind is None or e[0] == kind]
        read.reset = _abi.launch_log_reset
        yield read


# ---- stream / DTLS record layer harnesses -------------------------------------
def _al(x, a=128):
    return (x + a - 1) // a * a


ODD_IN_OFF = (1, 7, 13)      # Conns / Table encrypt(odd=True): in_off this far past the 128-aligned slot


def _send_layout(jobs, sizes, odd):
    """The descriptors and input arena of a send call: (d, ina, outs, pos_out, nmax)."""
    from mbedtls_amd import stream as S
    d = np.zeros(len(jobs), dtype=S.STREAM_OUT)
    ins, outs, pos_in, pos_out = [], [], 0, 0
    for i, ((slot, pt, ctr, frag, typ), size) in enumerate(zip(jobs, sizes)):
        shift = ODD_IN_OFF[i % 3] if odd else 0
        d[i]["in_off"], d[i]["in_len"], d[i]["slot"] = pos_in + shift, len(pt), slot
        d[i]["out_off"], d[i]["max_frag"], d[i]["type"] = pos_out, frag, typ
        d[i]["out_ctr"] = np.frombuffer(ctr if isinstance(ctr, bytes) else ctr.to_bytes(8, "big"), dtype=np.uint8)
        ins.append(pos_in + shift)
        outs.append((pos_out, size))
        pos_in += _al(len(pt) + 1 + shift)
        pos_out += _al(size + 1)
    # 0xEE between the contents: bytes read past a content's end that reach the output (as the inner type
    # byte or padding of a TLS 1.3 record, say) change it.  A read that is masked to the content's length
    # again cannot be seen in the output; the 128 B behind the last content only keep it inside the arena.
    ina = np.full(max(pos_in, 16) + 128, 0xEE if odd else 0, dtype=np.uint8)
    for (slot, pt, *_), o in zip(jobs, ins):
        ina[o:o + len(pt)] = np.frombuffer(pt, dtype=np.uint8)
    nmax = sum((len(j[1]) + (j[3] or 16384) - 1) // (j[3] or 16384) for j in jobs) + 1
    return d, ina, outs, pos_out, nmax


class Conns:
    """TLS streams.  slots: list of (cipher, version, key, iv, granularity); one key table."""

    def __init__(self, slots):
        self.slots = slots
        self.kt = M.KeyTable(len(slots))
        self.kt.load(np.concatenate([M.key_material(c, v, k, iv, g) for c, v, k, iv, g in slots]))
        self.ot = [O.Transform(v, c, k, k, iv, iv, granularity=g or 16) for c, v, k, iv, g in slots]

    def encrypt(self, jobs, odd=False):
        """jobs: list of (slot, plaintext, out_ctr(int), max_frag, type); odd:
        in_off at odd byte offsets (ODD_IN_OFF) instead of 128-aligned"""
        import torch
        from mbedtls_amd import stream as S
        sizes = [S.out_size(self.slots[j[0]][1], self.slots[j[0]][0], self.slots[j[0]][4], len(j[1]), j[3])
                 for j in jobs]
        d, ina, outs, pos_out, nmax = _send_layout(jobs, sizes, odd)
        dev = torch.device("cuda")
        tin = torch.from_numpy(ina).to(dev)
        tout = torch.zeros(max(pos_out, 16), dtype=torch.uint8, device=dev)
        recs = torch.zeros(nmax * 40, dtype=torch.uint8, device=dev)
        res = torch.zeros(nmax * 16, dtype=torch.uint8, device=dev)
        sres = torch.zeros(len(jobs) * 32, dtype=torch.uint8, device=dev)
        S.encrypt(self.kt, d, len(jobs), tin, tout, recs, res, nmax, sres)
        torch.cuda.synchronize()
        o = tout.cpu().numpy()
        sr = sres.cpu().numpy().view(S.STREAM_OUT_RES)
        self.last_regions = [o[p:p + size].tobytes() for p, size in outs]   # each job's whole output region
        return [(sr[i], o[p:p + int(sr[i]["out_len"])].tobytes()) for i, (p, _) in enumerate(outs)]

    def layout_in(self, conns):
        """conns: list of (slot, bytes, in_ctr(int), nb_zero) -> (descriptors, arena, offsets, record bound)"""
        from mbedtls_amd import stream as S
        d = np.zeros(len(conns), dtype=S.STREAM_IN)
        pos, offs = 0, []
        for i, (slot, data, ctr, nbz) in enumerate(conns):
            d[i]["off"], d[i]["len"], d[i]["slot"], d[i]["nb_zero"] = pos, len(data), slot, nbz
            d[i]["in_ctr"] = np.frombuffer(ctr.to_bytes(8, "big"), dtype=np.uint8)
            offs.append(pos)
            pos += _al(len(data) + 1)
        a = np.zeros(max(pos, 16), dtype=np.uint8)
        for (slot, data, *_), o in zip(conns, offs):
            a[o:o + len(data)] = np.frombuffer(data, dtype=np.uint8)
        return d, a, offs, sum(len(c[1]) // 6 + 1 for c in conns)

    def decrypt(self, conns):
        """conns: list of (slot, bytes, in_ctr(int), nb_zero)"""
        import torch
        from mbedtls_amd import stream as S
        d, a, offs, nmax = self.layout_in(conns)
        dev = torch.device("cuda")
        ta = torch.from_numpy(a).to(dev)
        recs = torch.zeros(nmax * 40, dtype=torch.uint8, device=dev)
        res = torch.zeros(nmax * 16, dtype=torch.uint8, device=dev)
        sres = torch.zeros(len(conns) * 32, dtype=torch.uint8, device=dev)
        S.decrypt(self.kt, d, len(conns), ta, recs, res, nmax, sres)
        torch.cuda.synchronize()
        return (ta.cpu().numpy(), recs.cpu().numpy().view(M.BATCH_REC), res.cpu().numpy().view(M.BATCH_RES),
                sres.cpu().numpy().view(S.STREAM_IN_RES), offs)

    def close(self):
        self.kt.close()


class Table:
    """DTLS 1.2 connections.  slots: list of (cipher, key, iv, cid) -- TLS 1.2
    keys; a slot with a CID is one direction (its out_cid when sending, in_cid
    when receiving)."""

    def __init__(self, slots, tls=M.VERSION_TLS1_2, tls_of=None, gran_of=None):
        """tls_of: {slot: version} for single slots that differ from `tls`;
        gran_of: {slot: padding granularity} (default 0 = 16)"""
        import torch
        self.slots = slots
        tls_of = tls_of or {}
        self.gran_of = gran_of or {}
        self.kt = M.KeyTable(len(slots))
        self.kt.load(np.concatenate([M.key_material(c, tls_of.get(s, tls), k, iv, self.gran_of.get(s, 0))
                                     for s, (c, k, iv, _) in enumerate(slots)]))
        self.ot = []
        for s, (c, k, iv, cid) in enumerate(slots):
            if cid:
                self.kt.set_cid(s, cid)
            t = O.Transform(O.TLS1_2 if tls_of.get(s, tls) == M.VERSION_TLS1_2 else O.TLS1_3, c, k, k, iv, iv,
                            granularity=self.gran_of.get(s, 0) or 16)
            t.set_cid(cid, cid)
            self.ot.append(t)
        torch.cuda.synchronize()

    def encrypt(self, jobs, odd=False):
        """jobs: (slot, plaintext, out_ctr bytes, max_frag, type) -> [(res, datagram bytes back to back, recs, res)];
        odd: as Conns.encrypt"""
        import torch
        from mbedtls_amd import dtls as D
        from mbedtls_amd import stream as S
        sizes = [D.out_size(self.slots[j[0]][0], self.gran_of.get(j[0], 0), len(self.slots[j[0]][3]), len(j[1]), j[3])
                 for j in jobs]
        d, ina, outs, pos_out, nmax = _send_layout(jobs, sizes, odd)
        dev = torch.device("cuda")
        tin = torch.from_numpy(ina).to(dev)
        tout = torch.zeros(max(pos_out, 16), dtype=torch.uint8, device=dev)
        recs = torch.zeros(nmax * 40, dtype=torch.uint8, device=dev)
        res = torch.zeros(nmax * 16, dtype=torch.uint8, device=dev)
        sres = torch.zeros(len(jobs) * 32, dtype=torch.uint8, device=dev)
        D.encrypt(self.kt, d, len(jobs), tin, tout, recs, res, nmax, sres)
        torch.cuda.synchronize()
        o = tout.cpu().numpy()
        sr = sres.cpu().numpy().view(S.STREAM_OUT_RES)
        rc = recs.cpu().numpy().view(M.BATCH_REC)
        rs = res.cpu().numpy().view(M.BATCH_RES)
        self.last_regions = [o[p:p + size].tobytes() for p, size in outs]   # each job's whole output region
        return [(sr[i], o[p:p + int(sr[i]["out_len"])].tobytes(), rc, rs) for i, (p, _) in enumerate(outs)]

    def layout_in(self, conns):
        """conns: (slot, dict of DtlsState fields, [datagram bytes]) ->
        (connection descriptors, datagram descriptors, datagrams, arena, offsets, record bound)"""
        from mbedtls_amd import dtls as D
        d = np.zeros(len(conns), dtype=D.DTLS_IN)
        dgl, pos, offs = [], 0, []
        for i, (slot, stt, dgs) in enumerate(conns):
            d[i]["first_dgram"], d[i]["ndgram"], d[i]["slot"] = len(dgl), len(dgs), slot
            d[i]["window_top"], d[i]["window"] = stt.get("window_top", 0), stt.get("window", 0)
            d[i]["badmac_seen"], d[i]["badmac_limit"] = stt.get("badmac_seen", 0), stt.get("badmac_limit", 0)
            d[i]["in_epoch"], d[i]["cid_len"], d[i]["nb_zero"] = stt.get("in_epoch", 0), stt.get("cid_len", 0), \
                stt.get("nb_zero", 0)
            d[i]["flags"] = (M.DTLS_ANTI_REPLAY if stt.get("anti_replay", 1) else 0) | \
                (M.DTLS_IGNORE_UNEXPECTED_CID if stt.get("ignore_unexpected_cid", 0) else 0)
            o = []
            for g in dgs:
                dgl.append((pos, len(g)))
                o.append(pos)
                pos += _al(len(g) + 3) + 16 * (len(dgl) % 3)     # assorted alignments
            offs.append(o)
        a = np.zeros(max(pos, 16), dtype=np.uint8)
        for (slot, stt, dgs), o in zip(conns, offs):
            for g, p in zip(dgs, o):
                a[p:p + len(g)] = np.frombuffer(g, dtype=np.uint8)
        dg = np.zeros(max(1, len(dgl)), dtype=D.DGRAM)
        for k, (p, L) in enumerate(dgl):
            dg[k]["off"], dg[k]["len"] = p, L
        nmax = sum(len(g) // 13 + 1 for c in conns for g in c[2]) + 1
        return d, dg, len(dgl), a, offs, nmax

    def decrypt(self, conns):
        """conns: (slot, dict of DtlsState fields, [datagram bytes])"""
        import torch
        from mbedtls_amd import dtls as D
        d, dg, ndg, a, offs, nmax = self.layout_in(conns)
        dev = torch.device("cuda")
        ta = torch.from_numpy(a).to(dev)
        recs = torch.zeros(nmax * 40, dtype=torch.uint8, device=dev)
        res = torch.zeros(nmax * 16, dtype=torch.uint8, device=dev)
        disp = torch.zeros(nmax, dtype=torch.int32, device=dev)
        cres = torch.zeros(len(conns) * 48, dtype=torch.uint8, device=dev)
        D.decrypt(self.kt, d, len(conns), dg, ndg, ta, recs, res, disp, nmax, cres)
        torch.cuda.synchronize()
        return (ta.cpu().numpy(), recs.cpu().numpy().view(M.BATCH_REC), res.cpu().numpy().view(M.BATCH_RES),
                disp.cpu().numpy(), cres.cpu().numpy().view(D.DTLS_IN_RES), offs)

    def close(self):
        self.kt.close()


def check_vs_oracle(tab, conns, got, skip=()):
    """a Table.decrypt result against oracle/dtls.c, connection by connection
    (skip: indices the caller checks itself)"""
    a, recs, res, disp, cres, offs = got
    for i, (slot, stt, dgs) in enumerate(conns):
        if i in skip:
            continue
        st = O.DtlsState()
        st.anti_replay = stt.get("anti_replay", 1)
        for f in ("window_top", "window", "badmac_seen", "badmac_limit", "in_epoch", "cid_len",
                  "ignore_unexpected_cid", "nb_zero"):
            if f in stt:
                setattr(st, f, stt[f])
        want, wrecs, after = O.dtls_decrypt(tab.ot[slot], st, dgs)
        g = cres[i]
        assert (int(g["status"]), int(g["nrec"]), int(g["naccepted"]), int(g["dgrams_done"]),
                int(g["invalid_dgrams"])) == (want["status"], want["nrec"], want["naccepted"],
                                              want["dgrams_done"], want["invalid_dgrams"]), (i, want)
        assert (int(g["window_top"]), int(g["window"]), int(g["badmac_seen"]), int(g["nb_zero"])) == \
            (st.window_top, st.window, st.badmac_seen, st.nb_zero), i
        f = int(g["first"])
        for k, (dgi, off, doff, dlen, dsp, typ) in enumerate(wrecs):
            assert int(disp[f + k]) == dsp, (i, k, dsp, int(disp[f + k]))
            assert int(recs[f + k]["buf_off"]) == offs[i][dgi] + off, (i, k)
            if dsp in (M.DTLS_DROPPED, M.DTLS_NOT_REACHED, M.ERR_SSL_UNEXPECTED_RECORD):
                # never decrypted by the reference: no plaintext may be left
                # (each byte is the received one, or wiped to zero)
                s0 = offs[i][dgi] + off
                got_b = a[s0:s0 + doff + dlen]
                rx = np.frombuffer(after[dgi][off:off + doff + dlen], dtype=np.uint8)
                assert ((got_b == rx) | (got_b == 0)).all(), (i, k, dsp)
            if dsp == 0:
                r = res[f + k]
                assert (int(r["data_offset"]), int(r["data_len"]), int(r["type"])) == (doff, dlen, typ), (i, k)
                s0 = offs[i][dgi] + off + doff
                assert a[s0:s0 + dlen].tobytes() == after[dgi][off + doff:off + doff + dlen], (i, k)
