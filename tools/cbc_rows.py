"""The AES-CBC + HMAC rows of tools/bench_stream.py and tools/bench_dtls.py
(--cbc): C connections x R records of `content` bytes under AES-128-CBC +
HMAC-SHA256, MAC-then-encrypt and encrypt-then-MAC, through the framed calls
(tlsrec_stream_*_ex / tlsrec_dtls_*_ex with TLSREC_FRAME_CBC), send and
receive.  The yardstick is taken in the same run: the plain batch call
(tlsrec_batch_encrypt / _decrypt) over the very record descriptors the framed
call wrote, on the same bytes.  A framed row should reach GATE of that rate
(framing and finish ~0.15 ms, the send copy pass ~1 ms, against ~23 ms of
batch for 1 M records: under 6 %).  One JSON line per (MAC order, direction);
a sample of connections is checked against the model of tests/cbc_frames_ref.py.
"""
import json
import time

import numpy as np

GATE = 0.9


def run(a, dtls):
    from tools import rowlib
    import torch
    import mbedtls_amd as M
    from mbedtls_amd import cbc as CB
    from mbedtls_amd import dtls as D
    from mbedtls_amd import stream as S
    from tests.prng import prng_array
    dev = torch.device("cuda")
    C, R, L = a.conns, a.recs, a.content
    mac, cipher = CB.MAC_SHA256, CB.CIPHER_AES_128_CBC
    n = C * R
    per_in = R * L
    raw = prng_array(0xCBC5, C * 48).reshape(C, 48)
    hdr = 13 if dtls else 5
    mod = D if dtls else S
    for etm in (0, 1):
        km = np.zeros(C, dtype=CB.CBC_KEY_MATERIAL)
        km["cipher"], km["tls_minor"], km["mac"], km["etm"] = cipher, 3, mac, etm
        km["key"][:, :16] = raw[:, :16]
        km["mac_key"][:, :32] = raw[:, 16:48]
        kt = M.KeyTable(C)
        CB.load(kt, km)
        per_out = (D.out_size_cbc(mac, etm, 0, per_in, L) if dtls else S.out_size_cbc(mac, etm, per_in, L))
        wire = per_out // R
        stride_in, stride_out = (per_in + 127) // 128 * 128, (per_out + 127) // 128 * 128
        tin = torch.randint(0, 256, (C * stride_in,), dtype=torch.uint8, device=dev)
        tout = torch.zeros(C * stride_out, dtype=torch.uint8, device=dev)
        ivs = torch.randint(0, 256, (16 * n,), dtype=torch.uint8, device=dev)
        d = np.zeros(C, dtype=S.STREAM_OUT)
        d["in_off"] = np.arange(C, dtype=np.uint64) * stride_in
        d["in_len"], d["slot"], d["type"], d["max_frag"] = per_in, np.arange(C), 23, L
        d["out_off"] = np.arange(C, dtype=np.uint64) * stride_out
        if dtls:
            d["out_ctr"][:, 1] = 1                                # epoch 1, sequence 0
        dout = torch.from_numpy(d.view(np.uint8).copy()).to(dev)
        recs = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
        res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        res2 = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        disp = torch.zeros(n, dtype=torch.int32, device=dev)
        sres = torch.zeros(C * 32, dtype=torch.uint8, device=dev)
        cres = torch.zeros(C * 48, dtype=torch.uint8, device=dev)
        opts = S.frame_opts(cbc_ivs=ivs)

        def wall(fn, prep=None):
            ts = []
            for k in range(a.steps + 1):
                if prep:
                    prep()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            return float(np.mean(ts[1:]))

        # ---- send: the framed call, then the batch call over the descriptors it wrote
        def framed_send():
            mod.encrypt_ex(kt, dout, C, tin, tout, recs, res, n, sres, opts)
        t_fs = wall(framed_send)
        ms_fs, _ = rowlib.event_timed(framed_send, a.steps)
        so = sres.cpu().numpy().view(S.STREAM_OUT_RES)
        assert (so["status"] == 0).all() and (so["out_len"] == per_out).all()
        sealed = tout.clone()
        ok = _check_sample(dtls, km, etm, tin, sealed, ivs, C, R, L, stride_in, stride_out, per_in, per_out)
        # (the records hold ciphertext now: CBC + HMAC over it is the same work)

        def batch_send():
            M.batch_encrypt(kt, recs, res2, n, tout, tout)
        t_bs = wall(batch_send)
        ms_bs, _ = rowlib.event_timed(batch_send, a.steps)
        assert (res2.cpu().numpy().view(M.BATCH_RES)["status"] == 0).all()

        # ---- receive: decrypt the sealed records in place (a fresh copy each step)
        work = torch.empty_like(sealed)
        if dtls:
            dg = np.zeros(n, dtype=D.DGRAM)
            dg["off"] = (np.arange(C, dtype=np.uint64)[:, None] * stride_out
                         + np.arange(R, dtype=np.uint64)[None, :] * wire).reshape(-1)
            dg["len"] = wire
            di = np.zeros(C, dtype=D.DTLS_IN)
            di["first_dgram"], di["ndgram"], di["slot"] = np.arange(C) * R, R, np.arange(C)
            di["in_epoch"], di["flags"] = 1, M.DTLS_ANTI_REPLAY
            tdg = torch.from_numpy(dg.view(np.uint8).copy()).to(dev)
        else:
            di = np.zeros(C, dtype=S.STREAM_IN)
            di["off"] = np.arange(C, dtype=np.uint64) * stride_out
            di["len"], di["slot"] = per_out, np.arange(C)
        din = torch.from_numpy(di.view(np.uint8).copy()).to(dev)
        ro = S.frame_opts()

        def framed_recv():
            if dtls:
                D.decrypt_ex(kt, din, C, tdg, n, work, recs, res, disp, n, cres, ro)
            else:
                S.decrypt_ex(kt, din, C, work, recs, res, n, sres, ro)

        def fresh():
            work.copy_(sealed)
        t_fr = wall(framed_recv, fresh)
        ms_fr, _ = rowlib.event_timed(framed_recv, a.steps, prep=fresh)
        if dtls:
            ci = cres.cpu().numpy().view(D.DTLS_IN_RES)
            assert (ci["status"] == 0).all() and (ci["naccepted"] == R).all()
        else:
            si = sres.cpu().numpy().view(S.STREAM_IN_RES)
            assert (si["status"] == 0).all() and (si["nrec"] == R).all()
        rr = res.cpu().numpy().view(M.BATCH_RES)
        assert (rr["data_len"] == L).all() and (rr["data_offset"] == hdr + 16).all()
        # plaintext of the sampled connections is the application data
        for i in (0, C // 2, C - 1):
            for k in (0, R - 1):
                o = i * stride_out + k * wire + hdr + 16
                ok &= bool((work[o:o + L] == tin[i * stride_in + k * L:i * stride_in + (k + 1) * L]).all())

        def batch_recv():                                         # the descriptors the framed receive wrote
            M.batch_decrypt(kt, recs, res2, n, work, work)
        t_br = wall(batch_recv, fresh)
        ms_br, _ = rowlib.event_timed(batch_recv, a.steps, prep=fresh)
        assert (res2.cpu().numpy().view(M.BATCH_RES)["status"] == 0).all()

        payload = float(C) * per_in
        proto = "DTLS 1.2" if dtls else "TLS 1.2 stream"
        for leg, tf, msf, tb, msb in (("send", t_fs, ms_fs, t_bs, ms_bs), ("receive", t_fr, ms_fr, t_br, ms_br)):
            ratio = tb / tf
            print(json.dumps({
                "metric": f"{proto} framed AES-128-CBC + HMAC-SHA256 {leg} throughput (device-resident, "
                          "TLSREC_FRAME_CBC, framing included)",
                "value": round(payload / tf / 2**30, 3), "unit": "GiB/s", "records_per_s": round(n / tf),
                "ms_per_call": round(tf * 1e3, 3), "gpu_ms_per_call": round(msf, 4),
                "config": {"connections": C, "records_per_connection": R, "content_bytes": L, "cipher": cipher,
                           "mac": mac, "etm": etm, "protocol": proto, "leg": leg},
                "batch_same_run": {"value": round(payload / tb / 2**30, 3), "unit": "GiB/s",
                                   "ms_per_call": round(tb * 1e3, 3), "gpu_ms_per_call": round(msb, 4),
                                   "what": "tlsrec_batch_" + ("encrypt" if leg == "send" else "decrypt") +
                                           " over the descriptors the framed call wrote, in place"},
                "ratio_to_batch": round(ratio, 4), "gate": GATE, "meets_gate": bool(ratio >= GATE),
                "timing": "wall time of the call + stream synchronize, mean of the steps after a warm-up call; "
                          "gpu_ms: HIP events on the call's stream",
                "check": {"model_sample_ok": bool(ok)}}), flush=True)
        kt.close()


def _check_sample(dtls, km, etm, tin, sealed, ivs, C, R, L, stride_in, stride_out, per_in, per_out):
    """three connections' wire bytes against the framing model over the CBC record model"""
    from tests import cbc_frames_ref as F
    from tests import cbc_ref as RF
    iv_np = None
    ok = True
    for i in (0, C // 2, C - 1):
        key = RF.Key(int(km["cipher"][i]), int(km["mac"][i]), etm, bytes(km["key"][i][:16]), bytes(km["mac_key"][i][:32]))
        if iv_np is None:
            iv_np = ivs.cpu().numpy()
        p = F.CbcProtector(key, lambda k, i=i: iv_np[16 * (i * R + k):16 * (i * R + k) + 16].tobytes())
        pt = tin[i * stride_in:i * stride_in + per_in].cpu().numpy().tobytes()
        c8 = (bytes([0, 1]) + bytes(6)) if dtls else bytes(8)
        st, want, _, _ = (F.dtls_encrypt if dtls else F.stream_encrypt)(p, pt, 23, c8, L)
        ok &= st == 0 and sealed[i * stride_out:i * stride_out + per_out].cpu().numpy().tobytes() == want
    return ok
