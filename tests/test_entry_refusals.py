"""GPU test of the refusal codes of the twelve whole-path entries -- sd_diarize, sd_activity and sd_voiceprint, each as device pcm (_dev), host pcm,
_f32 and _wav -- through the C ABI.  No network runs: every call is refused in front of it.  Whatever a case does not test is valid: a 5 s buffer,
kind SD_ACTIVITY_SPEECH, no spans, every output pointer set."""
import ctypes as C
import struct

import numpy as np
import pytest

import sdhip

pytestmark = pytest.mark.gpu

ARG, MODEL, SHORT = 1, 3, 4
FAMILIES = ("diarize", "activity", "voiceprint")
FORMS = ("dev", "pcm", "f32", "wav")
N5 = 80000


def _wav(n, bits=16, sr=16000):
    data = b"\x05" * (n * bits // 8)
    fmt = struct.pack("<HHIIHH", 1, 1, sr, sr * bits // 8, bits // 8, bits)
    return b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(data)) + data


@pytest.fixture(scope="module")
def sources(tmp_path_factory):
    import torch
    d = tmp_path_factory.mktemp("refusals")
    files = {"ok": _wav(N5), "missing": None, "bits24": _wav(100, bits=24), "empty16": _wav(0), "empty8": _wav(0, bits=8), "r44": _wav(N5, sr=44100),
             "empty44": _wav(0, sr=44100), "one": _wav(1)}
    for name, data in files.items():
        if data is not None:
            (d / (name + ".wav")).write_bytes(data)
    dev = torch.zeros(N5, dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    return {"dev": dev.data_ptr(), "pcm": np.zeros(N5, np.int16), "f32": np.zeros(N5, np.float32), "wav": {k: str(d / (k + ".wav")).encode() for k in files}, "keep": dev}


@pytest.fixture(scope="module")
def no_embedding_model(weights):
    d = sdhip.Diarizer(weights[0], None)
    yield d
    d.close()


# (form, what is wrong, code): the table of the twelve entries, the same for each family
INPUTS = [("dev", "null", ARG), ("dev", "n=0", SHORT), ("dev", "n=-5", SHORT), ("dev", "n=1", SHORT)]
INPUTS += [(f, w, ARG) for f in ("pcm", "f32") for w in ("null", "n=0", "n=-5")] + [("pcm", "n=1", SHORT), ("f32", "n=1", SHORT)]
INPUTS += [("wav", w, ARG) for w in ("null", "flags=8", "missing", "bits24", "empty16", "empty8", "r44")] + [("wav", "empty44+resample", SHORT), ("wav", "one", SHORT)]
CASES = [(fam, form, what, code) for fam in FAMILIES for form, what, code in INPUTS]
CASES += [(fam, form, out, ARG) for fam in ("diarize", "activity") for form in FORMS for out in ("turns=null", "n_turns=null")]
CASES += [("activity", form, "kind=2", ARG) for form in FORMS] + [("voiceprint", form, "h_emb=null", ARG) for form in FORMS]
CASES += [("voiceprint", "dev", "no model, n=0", SHORT), ("voiceprint", "dev", "no model", MODEL)]      # the length is tested first


@pytest.mark.parametrize("family,form,what,code", CASES, ids=["%s_%s %s" % (fam, form, what) for fam, form, what, _ in CASES])
def test_refusal_code(diarizer, no_embedding_model, sources, family, form, what, code):
    L = sdhip.lib()
    d = no_embedding_model if what.startswith("no model") else diarizer
    if form == "wav":
        name = what.split("+")[0] if what.split("+")[0] in sources["wav"] else "ok"
        src = None if what == "null" else sources["wav"][name]
        second = 8 if what == "flags=8" else 1 if what.endswith("+resample") else 0                    # the flags
    else:
        src = None if what == "null" else sources[form].ctypes.data if form != "dev" else sources["dev"]
        second = int(what.split("n=")[1]) if "n=" in what else N5                                       # the sample count
    turns, nt = C.POINTER(sdhip.Turn)(), C.c_int64(-1)
    p_turns = None if what == "turns=null" else C.byref(turns)
    p_nt = None if what == "n_turns=null" else C.byref(nt)
    emb, nw = (C.c_double * 192)(), C.c_int64(-1)
    fn = getattr(L, "sd_" + family + {"dev": "_dev", "pcm": "", "f32": "_f32", "wav": "_wav"}[form])
    if family == "diarize":
        rc = fn(d._h, src, second, p_turns, p_nt)
    elif family == "activity":
        rc = fn(d._h, src, second, 2 if what == "kind=2" else 0, p_turns, p_nt)
    else:
        rc = fn(d._h, src, second, None, 0, -1, None if what == "h_emb=null" else emb, C.byref(nw))
    msg = L.sd_last_error(d._h).decode()
    print("%s_%s %s: %d %s" % (family, form, what, rc, msg))
    assert rc == code
    assert msg
    if form == "pcm" and code == ARG:
        assert "sd_" + family in msg
    assert not turns                                   # nothing was handed over
