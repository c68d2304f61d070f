"""snarkjs.wtns.check (reference src/wtns_check.js) on the device: does the witness satisfy every constraint of the r1cs?

    ok = check(r1cs, wtns, logger)                  # each argument: bytes or a path; the reference's lines on logger.info / logger.warn, its verdict
    with Checker(r1cs) as c:                        # the layout of the constraints stays resident
        c.check(witness)                            # True | False
        c.check_many([w0, w1, ...])                 # per witness: index of the first failing constraint, or None
        c.check_dev(d_ptr, n)                       # the same for n witnesses already in device memory

Everything per constraint is ONE library call over a resident layout (include/zkmi.h: zkmi_r1cs_load, zkmi_r1cs_check; kernels in csrc/r1cs_check.cuh); this module
reads the two files as the reference does, words its lines and errors, and hands over the bytes. A constraint holds iff evalA * evalB == evalC in Fr, with the last
coefficient the file gives for a repeated signal and every 256-bit value taken mod r.

What the reference throws, check() raises as WtnsCheckError with the reference's message, after the same lines. Two things differ by necessity:
  * with no logger and a bad witness the reference dies on `logger.warn` (a TypeError); check() raises WtnsCheckError("Cannot read property 'warn' of undefined");
  * where the reference reads beyond a buffer (a constraint section that ends inside a record, a signal id at or beyond the witness's length) its verdict comes from
    whatever its memory held; check() raises WtnsCheckError instead, after the lines the reference logs before its loop. A section that ends inside a term COUNT
    makes the reference throw a RangeError once it gets there: check() raises that message, unless an earlier constraint fails, which is reported as the reference does.
"""
import ctypes as C
import os
import struct

import numpy as np

from . import zkmi
from .groth16_setup import SetupError, _Source, read_r1cs_header, read_sections

R_OF = {
    21888242871839275222246405745257275088548364400416034343698204186575808495617: ("bn128", 0),
    52435875175126190479447740508185965837690552500527637822603658699938581184513: ("bls12381", 1),
}
NONE = 0xFFFFFFFF
PROGRESS_EVERY = 500000


class WtnsCheckError(Exception):
    """wtns.check threw (the message is the reference's), or the inputs make the reference read beyond a buffer"""


class DeviceRefusal(Exception):
    """the device refused to load the constraints (a section that ends early, a signal id beyond nVars)"""


def progress_indices(n_constraints, first_bad):
    """the i of the reference's `··· processing r1cs constraints i/n` lines: every positive multiple of 500000 the loop reaches, i.e. up to the constraint it
    stopped at (first_bad) or, when every constraint holds, up to n_constraints - 1"""
    stop = n_constraints - 1 if first_bad is None else first_bad
    return list(range(PROGRESS_EVERY, stop + 1, PROGRESS_EVERY))


_next_key = [0x57c0000000000000]


class Device:
    """the library calls; a test replaces this class (tests/wtns_check_vectors.py: RestatedDevice)"""

    def load(self, curve, constraints, n_constraints, n_vars):
        """constraints: bytes-like or a list of them -> key of the resident layout"""
        zkmi.init()
        _next_key[0] += 1
        key = _next_key[0]
        pages = zkmi.pages_of(constraints)
        rc = zkmi.lib().zkmi_r1cs_load(zkmi.CURVE_ID[curve], pages.pages, n_constraints, n_vars, key)
        if rc == 2:
            raise DeviceRefusal(zkmi.lib().zkmi_last_error().decode(errors="replace"))
        zkmi.check(rc)
        return key

    def check(self, key, witnesses, n_witnesses):
        w = zkmi.u8(witnesses)
        out = np.empty(max(n_witnesses, 1), np.uint32)
        zkmi.check(zkmi.lib().zkmi_r1cs_check(key, zkmi.ptr(w), w.size, n_witnesses, zkmi.ptr(out)))
        return [int(v) for v in out[:n_witnesses]]

    def check_dev(self, key, d_ptr, nbytes, n_witnesses):
        out = np.empty(max(n_witnesses, 1), np.uint32)
        zkmi.check(zkmi.lib().zkmi_r1cs_check_dev(key, C.c_void_p(d_ptr), nbytes, n_witnesses, zkmi.ptr(out)))
        return [int(v) for v in out[:n_witnesses]]

    def release(self, key):
        zkmi.lib().zkmi_r1cs_release(key)


def _open(src, magic, max_version):
    s = _Source(src)
    try:
        return s, read_sections(s, magic, max_version)
    except SetupError as e:
        s.close()
        raise WtnsCheckError(str(e))
    except struct.error:
        s.close()
        raise WtnsCheckError("read beyond the end of the file")


def _section(src, sections, typ, name):
    """binfileutils readSection / startReadUniqueSection"""
    if typ not in sections:
        raise WtnsCheckError(f"{name}: Missing section {typ}")
    if len(sections[typ]) > 1:
        raise WtnsCheckError(f"{name}: Section Duplicated {typ}")
    return sections[typ][0]


def read_r1cs(r1cs):
    """-> (header dict, bytes of section 2): what readBinFile + readR1csFd(loadConstraints: false) + readSection(2) give wtns.check"""
    src, sections = _open(r1cs, b"r1cs", 1)
    try:
        _section(src, sections, 1, "r1cs")
        try:
            head = read_r1cs_header(src, sections)
        except (SetupError, struct.error):
            raise WtnsCheckError("read beyond the end of the file")
        head["useCustomGates"] = 4 in sections and 5 in sections
        return head, (src, sections)
    except Exception:
        src.close()
        raise


def read_wtns_header(wtns):
    """src/wtns_utils.js readHeader -> (n8, q, nWitness), and the open file"""
    src, sections = _open(wtns, b"wtns", 2)
    try:
        off, ln = _section(src, sections, 1, "wtns")
        try:
            n8 = struct.unpack("<I", src.read(off, 4))[0]
            q = int.from_bytes(src.read(off + 4, n8), "little")
            n_witness = struct.unpack("<I", src.read(off + 4 + n8, 4))[0]
        except (SetupError, struct.error):
            raise WtnsCheckError("read beyond the end of the file")
        if ln != 8 + n8:
            raise WtnsCheckError("Invalid section size reading")
        return dict(n8=n8, q=q, nWitness=n_witness), (src, sections)
    except Exception:
        src.close()
        raise


def _read_body(handle, typ, name):
    src, sections = handle
    off, ln = _section(src, sections, typ, name)
    try:
        return src.read(off, ln)
    except SetupError as e:
        raise WtnsCheckError(str(e))


def _where_it_ends(constraints, n_constraints, n_vars):
    """host scan of a section the device refused: ("count", constraint) when the section ends inside a term count — the reference throws a RangeError on reaching that
    constraint —, else ("record" | "signal", constraint): it reads beyond a buffer there"""
    pos, size = 0, len(constraints)
    for l in range(3 * n_constraints):
        if pos + 4 > size:
            return "count", l // 3
        n = struct.unpack_from("<I", constraints, pos)[0]
        if pos + 4 + 36 * n > size:
            return "record", l // 3
        if n and int(np.frombuffer(constraints, np.uint8, 36 * n, pos + 4).reshape(n, 36)[:, :4].copy().view("<u4").max()) >= n_vars:
            return "signal", l // 3
        pos += 4 + 36 * n
    return None, n_constraints


def _prefix_len(constraints, n_full):
    pos = 0
    for _ in range(3 * n_full):
        pos += 4 + 36 * struct.unpack_from("<I", constraints, pos)[0]
    return pos


class Checker:
    """the constraints of one r1cs, resident on the device"""

    def __init__(self, r1cs, device=None):
        self.dev = device or Device()
        self.key = None
        self.head, handle = read_r1cs(r1cs)
        try:
            if self.head["prime"] not in R_OF:
                raise WtnsCheckError(f"Curve not supported: {self.head['prime']}")
            self.curve = R_OF[self.head["prime"]][0]
            body = _read_body(handle, 2, "r1cs")
        finally:
            handle[0].close()
        self.n_vars, self.n_constraints = self.head["nVars"], self.head["nConstraints"]
        try:
            self.key = self.dev.load(self.curve, body, self.n_constraints, self.n_vars)
        except DeviceRefusal as e:
            raise WtnsCheckError(str(e))

    def _bytes(self, witness):
        if isinstance(witness, (str, os.PathLike)) or bytes(witness[:4]) == b"wtns":
            head, handle = read_wtns_header(witness)
            try:
                if head["q"] != self.head["prime"]:
                    raise WtnsCheckError("Curve of the witness does not match the curve of the proving key")
                witness = _read_body(handle, 2, "wtns")
            finally:
                handle[0].close()
        w = bytes(witness)
        if len(w) != 32 * self.n_vars:
            raise WtnsCheckError(f"the witness holds {len(w)} bytes, the r1cs has {self.n_vars} signals of 32 bytes")
        return w

    def check_many(self, witnesses):
        """witnesses: wtns files (paths or bytes) or raw section-2 bytes of nVars x 32 -> per witness the first failing constraint, or None"""
        ws = [self._bytes(w) for w in witnesses]
        if not ws:
            return []
        got = self.dev.check(self.key, b"".join(ws), len(ws))
        return [None if v == NONE else v for v in got]

    def check(self, witness):
        return self.check_many([witness])[0] is None

    def check_dev(self, d_ptr, n_witnesses=1):
        """n_witnesses x nVars x 32 bytes at device pointer d_ptr"""
        got = self.dev.check_dev(self.key, d_ptr, n_witnesses * self.n_vars * 32, n_witnesses)
        return [None if v == NONE else v for v in got]

    def close(self):
        if self.key is not None:
            self.dev.release(self.key)
            self.key = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def check(r1cs, wtns, logger=None, device=None):
    """wtns.check: True when the witness satisfies every constraint, False (after the reference's three warn lines) when not"""
    dev = device or Device()
    info = (lambda t: logger.info(t)) if logger else (lambda t: None)
    info("WITNESS CHECKING STARTED")
    info("> Reading r1cs file")
    head, h_r1cs = read_r1cs(r1cs)
    try:
        info("> Reading witness file")
        wh, h_wtns = read_wtns_header(wtns)
        try:
            if head["prime"] != wh["q"]:
                raise WtnsCheckError("Curve of the witness does not match the curve of the proving key")
            witness = _read_body(h_wtns, 2, "wtns")
        finally:
            h_wtns[0].close()
        if head["prime"] not in R_OF:
            raise WtnsCheckError(f"Curve not supported: {head['prime']}")
        curve = R_OF[head["prime"]][0]
        constraints = _read_body(h_r1cs, 2, "r1cs")
    finally:
        h_r1cs[0].close()
    n, n_vars = head["nConstraints"], head["nVars"]
    for line in ("----------------------------", "  WITNESS CHECK", f"  Curve:          {curve}", f"  Vars (wires):   {n_vars}", f"  Outputs:        {head['nOutputs']}",
                 f"  Public Inputs:  {head['nPubInputs']}", f"  Private Inputs: {head['nPrvInputs']}", f"  Labels:         {head['nLabels']}", f"  Constraints:    {n}",
                 f"  Custom Gates:   {'true' if head['useCustomGates'] else 'false'}", "----------------------------", "> Checking witness correctness"):
        info(line)

    def run(cons, n_c, vars_):
        key = dev.load(curve, cons, n_c, vars_)
        try:
            got = dev.check(key, witness[:32 * vars_], 1)[0]
        finally:
            dev.release(key)
        return None if got == NONE else got

    throws = None
    # the reference indexes the witness by signal id and never looks at nVars: what bounds a signal id is the number of values the witness holds
    vars_ = len(witness) // 32
    try:
        first_bad = run(constraints, n, vars_)
    except DeviceRefusal:
        kind, at = _where_it_ends(constraints, n, vars_)
        if kind != "count":
            raise WtnsCheckError(f"constraint {at}: the reference reads beyond {'the witness' if kind == 'signal' else 'the constraint section'} here; its verdict is undefined")
        first_bad = run(constraints[:_prefix_len(constraints, at)], at, vars_) if at else None
        if first_bad is None:
            first_bad, throws = at, "Offset is outside the bounds of the DataView"
    for i in progress_indices(n, first_bad):
        info(f"··· processing r1cs constraints {i}/{n}")
    if throws:
        raise WtnsCheckError(throws)
    if first_bad is not None:
        if not logger:
            raise WtnsCheckError("Cannot read property 'warn' of undefined")
        logger.warn(f"··· aborting checking process at constraint {first_bad}")
        logger.warn("WITNESS IS NOT CORRECT")
        logger.warn("WITNESS CHECKING FINISHED UNSUCCESSFULLY")
        return False
    info("WITNESS IS CORRECT")
    info("WITNESS CHECKING FINISHED SUCCESSFULLY")
    return True
