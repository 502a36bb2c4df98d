"""Writes tests/golden/proof_id_kat.json: known answers of the proof ids and the batch Merkle root
(DESIGN §18).

* "given": the answers the contract was published with (computed with hashlib where it was written):
  the ids of proof 0 of proofs_n16.npz, untouched (compact) and with Z of L[0] set to p + 1 (raw),
  each without and with taux and mu, with their message lengths; and the roots over
  ids_k = SHA-256(bytes([k & 255, k >> 8])), k < count.  They are literals here, never recomputed.
* "sets": from the Python restatement (tests/proof_id_ref.py) alone, for each golden proof set and
  f = 0, 1: the SHA-256 over the concatenated ids, the number of raw proofs and the root.

The restatement must reproduce "given" or nothing is written.

    python tests/golden/make_proof_id.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import codec_ref as cr       # noqa: E402
import proof_id_ref as pr    # noqa: E402

P1 = [0xFFFFFFFFFFFFFFEE, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF]   # p + 1
GIVEN = {
    "ids": [
        dict(input="tampered", kind=1, f=0, message_bytes=1856, id="0f3dcc00ccb2c199ec18cf51c5aa37fc6de2c033011333ccfea34b081c620cc5"),
        dict(input="tampered", kind=1, f=1, message_bytes=1920, id="6d8e66387263c1519f5d90aed74b9d949b42d45794e2c452c275222e450b6b48"),
        dict(input="untouched", kind=0, f=0, message_bytes=928, id="9d501615fe5ff36e1631f9996c64495d8504c749102da447723ded4c74870029"),
        dict(input="untouched", kind=0, f=1, message_bytes=992, id="8e78a6bf2ef9cf0fa3d514614a7325f42898ca395b560865e1f20912d35148ea"),
    ],
    "roots": {
        "0": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
        "1": "d37300dc2c6e038a83ee197ca0e181a77f6875afd9f537d31ca4995876481319",
        "2": "04f89961dc9136b6f3c1f7b51a1d4bed9dd47e713b81fd6be8241f72663e992f",
        "3": "1a40fb6a7e1fccbe40993b03c1157e2f8e3c4af505db37925f5dc6adb747fb4e",
        "7": "f53bb4c774794b67f3c87f3a5c4734ee8e1f193fced013ff8163b8e32ffab32b",
        "257": "feadb4c7b1a3395932e3231e618af5d0552ce76f321fd1f78c149efb8cec1053",
    },
}
SETS = ("proofs_n16", "proofs_n64", "rpverify_n16", "rpverify_n64")


def given_inputs():
    """input name -> (n, arrs) of the one proof the "given" ids are about."""
    n, arrs, _ = cr.golden_set("proofs_n16")
    one = cr.take(arrs, np.arange(1))
    bad = cr.take(arrs, np.arange(1))
    bad["L"][0, 0, 8:12] = np.array(P1, np.uint64)
    return {"untouched": (n, one), "tampered": (n, bad)}


def check_given(oracle):
    """The restatement against the literals; returns the mismatches."""
    wrong = []
    inputs = given_inputs()
    for g in GIVEN["ids"]:
        n, arrs = inputs[g["input"]]
        kind, msg = pr.message(oracle, arrs, n, 0, bool(g["f"]))
        if (kind, len(msg), hashlib.sha256(msg).hexdigest()) != (g["kind"], g["message_bytes"], g["id"]):
            wrong.append((g["input"], g["f"], kind, len(msg), hashlib.sha256(msg).hexdigest()))
    for count, root in GIVEN["roots"].items():
        if pr.mth(pr.kat_ids(int(count))).hex() != root:
            wrong.append(("root", count))
    return wrong


def main():
    from oracle import pyoracle
    if not os.path.exists(pyoracle.ORACLE_SO):
        pyoracle.build()
    O = pyoracle.Oracle()
    wrong = check_given(O)
    assert not wrong, wrong
    kat = dict(given=GIVEN, sets={})
    for name in SETS:
        n, arrs, _ = cr.golden_set(name)
        for f in (0, 1):
            ids, kinds = pr.proof_ids(O, arrs, n, bool(f))
            kat["sets"][f"{name}_f{f}"] = dict(n=n, count=len(ids), f=f, raw_count=int(sum(kinds)),
                                               ids_sha256=hashlib.sha256(b"".join(ids)).hexdigest(), root=pr.mth(ids).hex())
    with open(os.path.join(HERE, "proof_id_kat.json"), "w") as f:
        json.dump(kat, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(kat, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
