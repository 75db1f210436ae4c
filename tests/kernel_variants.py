"""Every hot-path kernel instantiation a bank can select at create, one row per choice, with the recipe of a bank that selects it.

A bank's sample-loop (or burst-demodulator) kernel is picked from its flags (JAERO_FLAG_EBNO = E, JAERO_FLAG_CAPTURE_SYMBOLS = C), its rate
and its size (jaero_hip.hip choose_kernels, burst_host.h burst_create); the second kernel class (jaero_profile_kernel's `which` = 1) is the
coarse estimate of a continuous bank or k_trident of a burst bank.  `layout` is what the row forces through
jaero_debug_sample_loop_layout (0 = by size, 1 = one pair per workgroup, 2 = four pairs per workgroup): it only exists for the kernels
chosen by size (k_oqpsk_fb, k_msk_fb at 80 taps).

The template arguments are spelled out as `nm -C` prints them, on purpose: re-tuning a constant (FB_LDSN, MFB*_LDSN, MFB*_TB, MSK_LDSN_*,
BMSK_FB_LDSN_*) renames an instantiation, and this table has to change in the same commit (tests/test_kernel_variant_table.py compares it
with the library's symbols; tests/test_gpu_variants.py runs every row against the oracle)."""
from __future__ import annotations

from dataclasses import dataclass

# kernel families whose instantiations a bank chooses at create (the kernel-handle symbols of the library)
KERNEL_FAMILIES = ("k_oqpsk_fb", "k_msk_fb", "k_msk_samples", "k_burst_msk_fb", "k_burst_oqpsk_demod", "k_trident", "k_coarse6",
                   "k_coarse6_13", "k_coarse6_w8400")

# bank recipes: kind, bit rate, sample rate, coarse-estimate FFT power
FAMILIES = {
    "oqpsk_10500": dict(kind="oqpsk", fb=10500.0, Fs=48000.0, power=14),
    "oqpsk_8400": dict(kind="oqpsk", fb=8400.0, Fs=48000.0, power=14),
    "msk_1200": dict(kind="msk", fb=1200.0, Fs=48000.0, power=13),  # 80 taps
    "msk_600": dict(kind="msk", fb=600.0, Fs=48000.0, power=13),  # 160 taps
    "msk_1200_24k": dict(kind="msk", fb=1200.0, Fs=24000.0, power=13),  # 40 taps
    "msk_1200_12k": dict(kind="msk", fb=1200.0, Fs=12000.0, power=13),  # 20 taps
    "burst_oqpsk": dict(kind="burst_oqpsk", fb=10500.0, Fs=48000.0, power=13),
    "burst_msk_1200": dict(kind="burst_msk", fb=1200.0, Fs=48000.0, power=13),
    "burst_msk_600": dict(kind="burst_msk", fb=600.0, Fs=48000.0, power=13),
}


@dataclass(frozen=True)
class Variant:
    family: str  # key of FAMILIES
    ebno: bool  # JAERO_FLAG_EBNO (burst banks: no such template argument, always False here)
    capture: bool  # JAERO_FLAG_CAPTURE_SYMBOLS
    layout: int  # jaero_debug_sample_loop_layout
    kernel0: str  # jaero_debug_kernel_variant(which = 0): sample loop / burst demodulator
    kernel1: str  # jaero_debug_kernel_variant(which = 1): coarse estimate / k_trident

    @property
    def burst(self) -> bool:
        return FAMILIES[self.family]["kind"].startswith("burst")

    @property
    def id(self) -> str:
        flags = "" if self.burst else f"-E{int(self.ebno)}"
        return f"{self.family}{flags}-C{int(self.capture)}-L{self.layout}"


V = Variant
VARIANTS = [
    # 10.5 kbps OQPSK: front / back pairs, one or four per workgroup
    V("oqpsk_10500", False, False, 1, "k_oqpsk_fb<55, 36, false, false, 1, false>", "k_coarse6"),
    V("oqpsk_10500", False, True, 1, "k_oqpsk_fb<55, 36, false, true, 1, false>", "k_coarse6"),
    V("oqpsk_10500", True, False, 1, "k_oqpsk_fb<55, 36, true, false, 1, false>", "k_coarse6"),
    V("oqpsk_10500", True, True, 1, "k_oqpsk_fb<55, 36, true, true, 1, false>", "k_coarse6"),
    V("oqpsk_10500", False, False, 2, "k_oqpsk_fb<55, 36, false, false, 4, false>", "k_coarse6"),
    V("oqpsk_10500", False, True, 2, "k_oqpsk_fb<55, 36, false, true, 4, false>", "k_coarse6"),
    V("oqpsk_10500", True, False, 2, "k_oqpsk_fb<55, 36, true, false, 4, false>", "k_coarse6"),
    V("oqpsk_10500", True, True, 2, "k_oqpsk_fb<55, 36, true, true, 4, false>", "k_coarse6"),
    # 8400 bps OQPSK: the prefiltered input, the halves taking turns
    V("oqpsk_8400", False, False, 1, "k_oqpsk_fb<55, 36, false, false, 1, true>", "k_coarse6_w8400"),
    V("oqpsk_8400", False, True, 1, "k_oqpsk_fb<55, 36, false, true, 1, true>", "k_coarse6_w8400"),
    V("oqpsk_8400", True, False, 1, "k_oqpsk_fb<55, 36, true, false, 1, true>", "k_coarse6_w8400"),
    V("oqpsk_8400", True, True, 1, "k_oqpsk_fb<55, 36, true, true, 1, true>", "k_coarse6_w8400"),
    V("oqpsk_8400", False, False, 2, "k_oqpsk_fb<55, 36, false, false, 4, true>", "k_coarse6_w8400"),
    V("oqpsk_8400", False, True, 2, "k_oqpsk_fb<55, 36, false, true, 4, true>", "k_coarse6_w8400"),
    V("oqpsk_8400", True, False, 2, "k_oqpsk_fb<55, 36, true, false, 4, true>", "k_coarse6_w8400"),
    V("oqpsk_8400", True, True, 2, "k_oqpsk_fb<55, 36, true, true, 4, true>", "k_coarse6_w8400"),
    # 1200 bps MSK at 48 kHz (80 taps): one pair (MFB_LDSN, MFB1_TB) or four pairs (MFB4_LDSN, MFB4_TB) per workgroup
    V("msk_1200", False, False, 1, "k_msk_fb<80, 36, false, false, 1, 32>", "k_coarse6_13"),
    V("msk_1200", False, True, 1, "k_msk_fb<80, 36, false, true, 1, 32>", "k_coarse6_13"),
    V("msk_1200", True, False, 1, "k_msk_fb<80, 36, true, false, 1, 32>", "k_coarse6_13"),
    V("msk_1200", True, True, 1, "k_msk_fb<80, 36, true, true, 1, 32>", "k_coarse6_13"),
    V("msk_1200", False, False, 2, "k_msk_fb<80, 32, false, false, 4, 18>", "k_coarse6_13"),
    V("msk_1200", False, True, 2, "k_msk_fb<80, 32, false, true, 4, 18>", "k_coarse6_13"),
    V("msk_1200", True, False, 2, "k_msk_fb<80, 32, true, false, 4, 18>", "k_coarse6_13"),
    V("msk_1200", True, True, 2, "k_msk_fb<80, 32, true, true, 4, 18>", "k_coarse6_13"),
    # 600 bps MSK at 48 kHz (160 taps): two pairs per workgroup at every size
    V("msk_600", False, False, 0, "k_msk_fb<160, 72, false, false, 2, 64>", "k_coarse6_13"),
    V("msk_600", False, True, 0, "k_msk_fb<160, 72, false, true, 2, 64>", "k_coarse6_13"),
    V("msk_600", True, False, 0, "k_msk_fb<160, 72, true, false, 2, 64>", "k_coarse6_13"),
    V("msk_600", True, True, 0, "k_msk_fb<160, 72, true, true, 2, 64>", "k_coarse6_13"),
    # 40 and 20 taps: one wavefront per channel group
    V("msk_1200_24k", False, False, 0, "k_msk_samples<40, 24, false, false>", "k_coarse6_13"),
    V("msk_1200_24k", False, True, 0, "k_msk_samples<40, 24, false, true>", "k_coarse6_13"),
    V("msk_1200_24k", True, False, 0, "k_msk_samples<40, 24, true, false>", "k_coarse6_13"),
    V("msk_1200_24k", True, True, 0, "k_msk_samples<40, 24, true, true>", "k_coarse6_13"),
    V("msk_1200_12k", False, False, 0, "k_msk_samples<20, 12, false, false>", "k_coarse6_13"),
    V("msk_1200_12k", False, True, 0, "k_msk_samples<20, 12, false, true>", "k_coarse6_13"),
    V("msk_1200_12k", True, False, 0, "k_msk_samples<20, 12, true, false>", "k_coarse6_13"),
    V("msk_1200_12k", True, True, 0, "k_msk_samples<20, 12, true, true>", "k_coarse6_13"),
    # burst banks: the demodulator per capture flag, k_trident per kind
    V("burst_oqpsk", False, False, 0, "k_burst_oqpsk_demod<false>", "k_trident<true>"),
    V("burst_oqpsk", False, True, 0, "k_burst_oqpsk_demod<true>", "k_trident<true>"),
    V("burst_msk_1200", False, False, 0, "k_burst_msk_fb<false, 80, 48>", "k_trident<false>"),
    V("burst_msk_1200", False, True, 0, "k_burst_msk_fb<true, 80, 48>", "k_trident<false>"),
    V("burst_msk_600", False, False, 0, "k_burst_msk_fb<false, 160, 128>", "k_trident<false>"),
    V("burst_msk_600", False, True, 0, "k_burst_msk_fb<true, 160, 128>", "k_trident<false>"),
]
del V


def expected_symbols() -> set:
    """Every instantiation the table expects the library to hold."""
    return {v.kernel0 for v in VARIANTS} | {v.kernel1 for v in VARIANTS}


def find(family: str, ebno: bool, capture: bool, layout: int) -> Variant:
    (v,) = [v for v in VARIANTS if (v.family, v.ebno, v.capture, v.layout) == (family, ebno, capture, layout)]
    return v
