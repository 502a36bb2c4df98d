"""Writes tests/golden/codec_kat.json: the SHA-256 and byte length of the version-1 proof blobs of the
golden proof sets, from the Python restatement (tests/codec_ref.py) alone: proofs_n16 / proofs_n64
without taux and mu, rpverify.npz's n16 / n64 sets with them (their `rand` cases are raw).  The
digests pin the format: a change to the layout, the classification or the header changes them.

    python tests/golden/make_codec.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import codec_ref as cr   # noqa: E402

SETS = (("proofs_n16", False), ("proofs_n64", False), ("rpverify_n16", True), ("rpverify_n64", True))


def main():
    from oracle import pyoracle
    if not os.path.exists(pyoracle.ORACLE_SO):
        pyoracle.build()
    O = pyoracle.Oracle()
    kat = {}
    for name, blinding in SETS:
        n, arrs, _ = cr.golden_set(name)
        blob = cr.encode(O, arrs, n, blinding)
        m, back = cr.decode(O, blob)
        assert m == n and cr.same(arrs, back, list(back))
        raw = sum(0 if cr.is_compact(O, arrs, i) else 1 for i in range(len(arrs["V"])))
        kat[name] = dict(n=n, count=len(arrs["V"]), with_blinding=blinding, raw_count=raw, bytes=len(blob),
                         sha256=hashlib.sha256(blob).hexdigest())
    with open(os.path.join(HERE, "codec_kat.json"), "w") as f:
        json.dump(kat, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(kat, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
