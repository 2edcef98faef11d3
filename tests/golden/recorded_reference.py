"""What the reference's own compiled code (oracle/_ref) returned in the port-vs-reference tests, kept as SHA-256
digests so that those tests also run where oracle/_ref cannot be built (no reference tree at build time).

    agree_with_reference(oracle, key, port_arrays, ref_fn)

With oracle/_ref present the port's arrays are compared with ref_fn()'s bit for bit, as before, and the recorded
digest must equal the digest of ref_fn()'s arrays (the fixture still describes the reference).  Without it, the
digest of the port's arrays must equal the recorded one: bit-exact equality with the recorded reference result.
The digests are written by tests/golden/make_reference_digests.py, which runs the same tests in record mode.
"""
import hashlib
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_digests.json")
RECORD_ENV = "PD3_RECORD_REFERENCE_DIGESTS"


def digest(arrays):
    """SHA-256 over dtype, shape and bytes of every array, in order."""
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape};".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _load():
    if not os.path.exists(PATH):
        return {}
    with open(PATH) as f:
        return json.load(f)


def _beq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, a.shape, b.dtype, b.shape)
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


def agree_with_reference(oracle, key, port_arrays, ref_fn):
    port_arrays = [np.asarray(a) for a in port_arrays]
    if os.environ.get(RECORD_ENV):
        assert oracle.have_ref(), "recording needs oracle/_ref"
        ref = [np.asarray(a) for a in ref_fn()]
        for a, b in zip(port_arrays, ref, strict=True):
            _beq(a, b)
        table = _load()
        table[key] = digest(ref)
        with open(PATH, "w") as f:
            json.dump(dict(sorted(table.items())), f, indent=1)
            f.write("\n")
        return
    want = _load().get(key)
    assert want is not None, f"no recorded reference digest for {key!r} (tests/golden/make_reference_digests.py)"
    if oracle.have_ref():
        ref = [np.asarray(a) for a in ref_fn()]
        for a, b in zip(port_arrays, ref, strict=True):
            _beq(a, b)
        assert digest(ref) == want, f"{key}: oracle/_ref no longer gives the recorded result"
    assert digest(port_arrays) == want, f"{key}: the port differs from the recorded reference result"
