"""CPU-side checks of the batch key derivation for the AES-CBC + HMAC suites
(include/tlsrec.h, tlsrec_tls12_keytab_derive_cbc): both builds of the library
export it, the Python binding declares it, and a NULL table is refused before
any device is looked at.  No test here needs a device."""
import subprocess

import mbedtls_amd as M
from mbedtls_amd import _abi
from mbedtls_amd import cbc as C
from mbedtls_amd import tls12 as T

NAME = "tlsrec_tls12_keytab_derive_cbc"


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def test_both_libraries_export_the_call():
    for path in (_abi.LIB_PATH, _abi.TEST_LIB_PATH):
        names = _exports(path)
        assert NAME in names, path
        assert "tlsrec__tls12_stage_keys_cbc" in names, path      # the derive kernel alone (tools/bench_keysched.py)
    assert NAME in _abi.SIGNATURES and hasattr(M.load(), NAME)
    assert "tls12_keytab_derive_cbc" in T.__all__


def test_null_table_is_bad_input_without_a_gpu():
    """kt NULL comes first: whatever the other arguments are, and no device is touched"""
    fn = M.load().tlsrec_tls12_keytab_derive_cbc
    bad = M.ERR_SSL_BAD_INPUT_DATA
    ok = (C.CIPHER_AES_128_CBC, C.MAC_SHA256, 0, T.PRF_SHA256)
    assert fn(None, 0, 0, *ok, None, None) == bad
    assert fn(None, 0, 4, *ok, None, None) == bad
    assert fn(None, 0, 4, 0, 0, 7, T.PRF_NONE, None, None) == bad       # before the cipher, mac, prf and etm checks
    try:
        T.tls12_keytab_derive_cbc(None, 0, 1, *ok, None)
    except T.KeyScheduleError as e:
        assert e.code == bad
    else:
        raise AssertionError("a NULL table was accepted")
