#!/usr/bin/env python3
"""Writes tests/golden/jni_refusals.json: what the JNI shim, run under the fake JVM (tests/jni_fake.py), answers to every
refusal case of tests/test_jni_cpu.py -- exception class and message.  Our own recorded output; needs the built
lib/libmfsgd.so and no device.  Run it only when a refusal is changed on purpose."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

if __name__ == "__main__":
    from tests import jni_fake
    from tests import test_jni_cpu as t

    jvm = jni_fake.load()
    h = jvm.nativeCreate(t.U, t.I, t.K, t.LR, t.LAM, 0, 0)  # as the tests' `model`: ratings and seeded factors
    jvm.ok()
    t.Call(jvm, "nativeSetRatings", t.valid(h)["nativeSetRatings"]).close()
    jvm.nativeInitFactors(h, t.SEED)
    jvm.ok()
    out = t.recorded_refusals(jvm, h)
    jvm.nativeDestroy(h)
    with open(t.REFUSALS, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(out), "refusals recorded")
