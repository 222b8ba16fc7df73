"""-m gpu: what every *_device entry point of the known-image calls refuses about its member records before it launches
anything (include/ctmr.h; engine/image.inc known_open / known_bind): a null pointer to the records of
an image that has some, and a record count that is one off from the header's.  Import, query, remove, sort, image
lists, image resp, merge (operands A and B) and find (operands K and P), each called through the library with a valid
meta of two sets and three member records and ONE defect: CTMR_E_INVAL, and a message under the call's own name.
Both defects are found on the host: no kernel runs on the bad operand.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import known_image as KI, _native as N

DEV = torch.device("cuda:0")
DIGEST = bytes(range(32))
IMAGE = KI.build({KI.set_key(480000, DIGEST): [b"\x01", b"\x02\x03"], KI.set_key(480001, DIGEST): [b"\x04"]})
N_REC = 3
META, RECORDS = IMAGE[:-48 * N_REC], np.frombuffer(IMAGE[-48 * N_REC:], np.uint8)


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dev():
    """The three records (and one record of slack), and a scratch buffer for what a call would write."""
    rec = torch.from_numpy(np.concatenate([RECORDS, np.zeros(48, np.uint8)])).to(DEV)
    out = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    assert rec.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    return rec, out


def _one(name):
    """f(eng, d, n, good, out) → rc for the calls of one operand: d, n are the operand under test."""
    def import_(e, d, n, good, out):
        return e._lib.ctmr_known_import_device(e._h, META, len(META), d, n, 1, 0, C.byref(N.KnownImportStats()))

    def query(e, d, n, good, out):
        return e._lib.ctmr_known_query_device(e._h, META, len(META), d, n, 1, 0, out, 64, None, 0, C.byref(N.KnownProbeStats()))

    def remove(e, d, n, good, out):
        return e._lib.ctmr_known_remove_device(e._h, META, len(META), d, n, 1, 0, C.byref(N.KnownProbeStats()))

    def sort(e, d, n, good, out):
        return e._lib.ctmr_known_sort_device(e._h, META, len(META), d, n)

    def lists(e, d, n, good, out):
        ids, offs = np.zeros(256, np.uint8), np.zeros(16, np.uint64)
        return e._lib.ctmr_known_image_lists_device(e._h, META, len(META), d, n, 0, out, 4096, ids.ctypes.data, ids.size,
                                                    offs.ctypes.data, offs.size, C.byref(N.KnownListsInfo()))

    def resp(e, d, n, good, out):
        return e._lib.ctmr_known_image_resp_device(e._h, META, len(META), d, n, 512, out, 4096, C.byref(N.KnownRespInfo()))

    return {"import": import_, "query": query, "remove": remove, "sort": sort, "lists": lists, "resp": resp}[name]


def _two(name, second):
    """The calls of two operands: the one under test is the first (A, K) or the second (B, P), the other is good."""
    def merge(e, d, n, good, out):
        (da, na), (db, nb) = ((good, N_REC), (d, n)) if second else ((d, n), (good, N_REC))
        meta = np.zeros(1024, np.uint8)
        return e._lib.ctmr_known_merge_device(e._h, N.KNOWN_UNION, META, len(META), da, na,
                                              META, len(META), db, nb, meta.ctypes.data, meta.size, out, 4096 // 48,
                                              C.byref(N.KnownImageInfo()))

    def find(e, d, n, good, out):
        (dk, nk), (dp, np_) = ((good, N_REC), (d, n)) if second else ((d, n), (good, N_REC))
        hh = np.zeros(16 * 16, np.uint8)
        return e._lib.ctmr_known_image_find_device(e._h, META, len(META), dk, nk, META, len(META), dp, np_, 0, out, 16,
                                                   hh.ctypes.data, 16, C.byref(N.KnownFindInfo()))

    return {"merge": merge, "find": find}[name]


# entry point → (the call, its name in a count message, its name in a null-pointer message)
CALLS = {
    "import": (_one("import"), b"known import: ", b"known import: "),
    "query": (_one("query"), b"known query: ", b"known query: "),
    "remove": (_one("remove"), b"known remove: ", b"known remove: "),
    "sort": (_one("sort"), b"known sort: ", b"known sort: "),
    "image-lists": (_one("lists"), b"known image lists: ", b"known image lists: "),
    "image-resp": (_one("resp"), b"known image resp: ", b"known image resp: "),
    "merge-A": (_two("merge", False), b"known merge (A): ", b"known merge (A): "),
    "merge-B": (_two("merge", True), b"known merge (B): ", b"known merge (B): "),
    "find-K": (_two("find", False), b"known image find (K): ", b"known image find: "),
    "find-P": (_two("find", True), b"known image find (P): ", b"known image find: "),
}


@pytest.mark.parametrize("defect", ["null", "one-more", "one-less"])
@pytest.mark.parametrize("name", list(CALLS))
def test_a_device_operand_with_one_defect_is_refused(name, defect, eng, dev):
    f, count_prefix, null_prefix = CALLS[name]
    rec, out = dev
    good = C.c_void_p(rec.data_ptr())
    before = eng.total_count()
    if defect == "null":
        rc = f(eng, None, N_REC, good, C.c_void_p(out.data_ptr()))
        prefix, saying = null_prefix, b"null member records"
    else:
        n = N_REC + (1 if defect == "one-more" else -1)
        rc = f(eng, good, n, good, C.c_void_p(out.data_ptr()))
        prefix, saying = count_prefix, b"%d member records given, the header says %d" % (n, N_REC)
    msg = eng._lib.ctmr_last_error(eng._h)
    assert rc == N.E_INVAL, (rc, msg)
    assert msg.startswith(prefix) and saying in msg, msg
    assert eng.total_count() == before and not out.any().item(), "something was written"
    assert (rec.cpu().numpy()[:RECORDS.size] == RECORDS).all()
