"""powersOfTau.preparePhase2 and powersOfTau.convert on the device (src/powersoftau_preparephase2.js, src/powersoftau_convert.js): the Lagrange sections
12 - 15 a phase-2 setup reads, from the powers of tau of sections 2 - 5.

    new = prepare_phase2(old_ptau, new_ptau=None, logger=None)                       # old_ptau: bytes or a path; new_ptau: a path or None
    new = convert(old_ptau, new_ptau=None, logger=None)

Both return the new file's bytes, byte for byte what the reference writes, and also write them when a path is given. Everything on curve points is one
library call per section (include/zkmi.h):
    zkmi_ptau_lagrange_section  for p = first .. top the inverse group FFT of the first 2^p points of the section, all blocks from one upload in one pass
The reference makes one G.ifft per power and section, each with a re-read of the source section. Section 12 (tauG1) goes to top = power + 1 with the last
point of its top block taken as infinity: section 2 holds 2^(power + 1) - 1 points. The new header states ceremonyPower = power: the reference calls
writePTauHeader without a ceremony power. convert copies the old sections 12 - 15 and appends the power + 1 block to section 12, whether the old section
already holds it or not, as the reference does. The reference's logger receives debug lines only; they are not reproduced.
"""
import ctypes as C
import struct

import numpy as np

from . import zkmi
from .groth16_setup import CURVES, SetupError, _Source, read_sections
from .powersoftau_verify import PtauError


class Device:
    """the one call that needs the device; tests/test_ptau_prepare_host.py puts the CPU oracle in its place"""

    def lagrange_section(self, cv, group, tau, n_tau, first, top, zero_last):
        """tau: bytes or a list of pages -> the blocks first .. top back to back, 2^(top + 1) - 2^first points"""
        zkmi.init()
        s_g = 2 * group * cv["n8q"]
        n_out = ((2 << top) - (1 << first)) * s_g
        pt = zkmi.pages_of(tau)
        out = np.zeros(n_out, np.uint8)
        o_ptr, o_len = (C.c_void_p * 1)(out.ctypes.data), (C.c_size_t * 1)(n_out)
        zkmi.check(zkmi.lib().zkmi_ptau_lagrange_section(cv["id"], group, pt.pages, n_tau, first, top, 1 if zero_last else 0, o_ptr, o_len, 1))
        return out.tobytes()


def _open(src):
    """the sections and header of a well-formed file: sections 1 - 7 once each, with the sizes the header implies -> (sections, cv, power)"""
    try:
        sections = read_sections(src, b"ptau", 1)
    except (SetupError, struct.error) as e:
        raise PtauError(str(e)) from None
    for t in range(1, 8):
        if t not in sections:
            raise PtauError(f"ptau: Missing section {t}")
        if len(sections[t]) > 1:
            raise PtauError(f"ptau: Section Duplicated {t}")
    head = src.read(*sections[1][0])
    if len(head) < 4:
        raise PtauError("Invalid PTau header size")
    n8 = struct.unpack_from("<I", head, 0)[0]
    if len(head) != 4 + n8 + 8:
        raise PtauError("Invalid PTau header size")
    q = int.from_bytes(head[4:4 + n8], "little")
    if q not in CURVES:
        raise PtauError(f"Curve not supported: {q}")
    cv = CURVES[q]
    if cv["n8q"] != n8:
        raise PtauError("Invalid size")
    power = struct.unpack_from("<I", head, 4 + n8)[0]
    if power + 1 > cv["s"]:
        raise PtauError(f"power {power}: the tauG1 section needs a transform of 2^{power + 1} elements, beyond the limit of 2^{cv['s']} (Fr.s) of this curve")
    s1, s2 = 2 * n8, 4 * n8
    for t, size in ((2, ((2 << power) - 1) * s1), (3, (1 << power) * s2), (4, (1 << power) * s1), (5, (1 << power) * s1), (6, s2)):
        if sections[t][0][1] != size:
            raise PtauError("Invalid section size reading")
    return sections, cv, power


def _header(cv, power):
    """writePTauHeader(fd, curve, power): the ceremony power defaults to the power"""
    q = next(k for k, c in CURVES.items() if c is cv)
    return struct.pack("<I", cv["n8q"]) + q.to_bytes(cv["n8q"], "little") + struct.pack("<II", power, power)


def _file(secs):
    out = [b"ptau", struct.pack("<II", 1, len(secs))]
    for typ, body in secs:
        out += [struct.pack("<IQ", typ, len(body)), body]
    return b"".join(out)


def _finish(raw, new_ptau):
    if new_ptau is not None:
        with open(new_ptau, "wb") as f:
            f.write(raw)
    return raw


# (old section, new section, group, top - power, zero_last)
_LADDERS = ((2, 12, 1, 1, True), (3, 13, 2, 0, False), (4, 14, 1, 0, False), (5, 15, 1, 0, False))


def _prepare_phase2(old_ptau, new_ptau, logger, dev):
    src = _Source(old_ptau)
    try:
        sections, cv, power = _open(src)
        secs = [(1, _header(cv, power))] + [(t, src.read(*sections[t][0])) for t in range(2, 8)]
        for old, new, group, up, zero_last in _LADDERS:
            top = power + up
            tau = secs[old - 1][1]
            n_tau = (1 << top) - (1 if zero_last else 0)
            secs.append((new, dev.lagrange_section(cv, group, tau[:n_tau * 2 * group * cv["n8q"]], n_tau, 0, top, zero_last)))
    finally:
        src.close()
    return _finish(_file(secs), new_ptau)


def _convert(old_ptau, new_ptau, logger, dev):
    src = _Source(old_ptau)
    try:
        sections, cv, power = _open(src)
        for t in (12, 13, 14, 15):
            if t not in sections:
                raise PtauError(f"ptau: Missing section {t}")
            if len(sections[t]) > 1:
                raise PtauError(f"ptau: Section Duplicated {t}")
        secs = [(1, _header(cv, power))] + [(t, src.read(*sections[t][0])) for t in range(2, 8)]
        top = power + 1
        block = dev.lagrange_section(cv, 1, secs[1][1], (1 << top) - 1, top, top, True)
        secs.append((12, src.read(*sections[12][0]) + block))
        for t in (13, 14, 15):
            secs.append((t, src.read(*sections[t][0])))
    finally:
        src.close()
    return _finish(_file(secs), new_ptau)


def prepare_phase2(old_ptau, new_ptau=None, logger=None):
    """snarkjs.powersOfTau.preparePhase2(oldPtau, newPtau, logger) -> the new file's bytes"""
    return _prepare_phase2(old_ptau, new_ptau, logger, Device())


def convert(old_ptau, new_ptau=None, logger=None):
    """snarkjs.powersOfTau.convert(oldPtau, newPtau, logger) -> the new file's bytes"""
    return _convert(old_ptau, new_ptau, logger, Device())
