"""Histories of run_admm as JSON that keeps every bit: a float is its ``float.hex()``, an array the
list of its entries' (int64: the integers), a list or tuple the list of its items, None stays None.
Two values are bitwise equal exactly when their encodings are equal (every NaN encodes as 'nan').
The fixtures under tests/golden/ keep a scalar history (one float per iteration) as that encoding and an
array-valued one as ``digest`` of it -- 64 bits of its SHA-256 -- so that a recorded run stays a few
kilobytes; a changed bit anywhere changes what is stored for its history key."""
import hashlib
import json

import numpy as np


def encode(v):
    if v is None:
        return None
    if isinstance(v, np.ndarray):
        if v.dtype == np.int64:
            return {"int64": [int(e) for e in v.ravel()], "shape": list(v.shape)}
        assert v.dtype == np.float64, v.dtype
        return {"float64": [float(e).hex() for e in v.ravel()], "shape": list(v.shape)}
    if isinstance(v, (list, tuple)):
        return [encode(e) for e in v]
    assert type(v) is float, type(v)  # (a numpy scalar would be another type of history entry)
    return v.hex()


def digest(v) -> str:
    return hashlib.sha256(json.dumps(encode(v), separators=(",", ":")).encode()).hexdigest()[:16]


def digest_history(hist):
    """{key: the hex floats of a scalar history, the digest of an array-valued one}; every history is a
    plain list of per-iteration values."""
    for k, v in hist.items():
        assert type(v) is list, (k, type(v))
    return {k: encode(v) if all(type(e) is float for e in v) else digest(v) for k, v in hist.items()}


def dump(obj, path):
    """Write the fixture ``obj`` as JSON with one line per entry of its top-level dicts and lists (a case,
    a history key, an image), compact within the line."""
    def one(v):
        return json.dumps(v, sort_keys=True, separators=(",", ":"))

    lines = []
    for k in sorted(obj):
        v = obj[k]
        if isinstance(v, dict):
            body = ",\n".join(f"{one(s)}:{one(v[s])}" for s in sorted(v))
            lines.append(f"{one(k)}:{{\n{body}\n}}")
        elif isinstance(v, list):
            lines.append(f"{one(k)}:[\n" + ",\n".join(one(e) for e in v) + "\n]")
        else:
            lines.append(f"{one(k)}:{one(v)}")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")
