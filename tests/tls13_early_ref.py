"""The three steps of a resumed TLS 1.3 handshake over the hashlib ladder of
tests/tls13_ref.py: the checker of tests/test_tls13_early_cpu.py and
tests/test_tls13_early_gpu.py.  The PSK binder follows RFC 8446 4.2.11.2, the
early secrets the diagram of 7.1, the ticket PSK 4.6.1."""
from tests import tls13_ref as R


def early_stage(hname, psk, resumption, binder_transcript, hello_transcript, key_len):
    """One connection of tlsrec_tls13_keytab_derive_early (and, for its binder,
    of tlsrec_tls13_batch_psk_binder).  Returns a dict: early, binder, c_e,
    e_exp and keys, the (key, iv) of c e traffic."""
    early = R.evolve(hname, None, psk)
    bk = R.derive_secret(hname, early, b"res binder" if resumption else b"ext binder", b"", hashed=False)
    c_e = R.derive_secret(hname, early, b"c e traffic", hello_transcript)
    return {"early": early, "binder": R.calc_finished(hname, bk, binder_transcript), "c_e": c_e,
            "e_exp": R.derive_secret(hname, early, b"e exp master", hello_transcript),
            "keys": R.traffic_keys(hname, c_e, key_len)}


def ticket_psk(hname, res_master, nonce):
    """HKDF-Expand-Label(resumption_master_secret, "resumption", ticket_nonce, Hash.length)"""
    return R.expand_label(hname, res_master, b"resumption", nonce, R.HLEN[hname])
