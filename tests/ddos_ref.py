"""A numpy model of the entropy flood detector (rxg_ddos_dev / rxg_ddos_host),
written from the rule in include/rxgpu.h and not from the C++.

Per frame j: set_j = 1-bits in its len bytes, tot_j = 8 * len.
e(s, t) = (-s)*(log2 s - log2 t) - (t-s)*(log2(t-s) - log2 t) + log2 t.
Frame g (counted since the state was fresh) takes slot g mod 256; g < 256 is
warm-up (not checked, flag untouched); from g = 256 on the window g-255 .. g
gives S, T (u32), E = sum e, D = E - e(S, T), alarm = thresh < D.  A frame with
s == 0 or s >= t has no e: every window holding it is undefined (D NaN, no
alarm, the flag drops), decided from the integers.

The model keeps the whole history of (set, tot) it has seen, so a window is a
plain slice; sums are numpy's (pairwise), in float64 or, for the error
estimate, longdouble.  tol(g) is the worst-case bound of 256 sequential f64
adds plus a few ulps per term: 512 * 2^-52 * (sum_window tot*log2 tot +
T*log2 T)."""
import numpy as np

WINDOW = 256
WARMUP, UNDEF, ALARM, RISE, FALL = 0x01, 0x02, 0x04, 0x08, 0x10
NO_ALARM = 0xFFFFFFFF
STATE_DTYPE = np.dtype([("frames_seen", "<u8"), ("flag", "<u4"), ("_r0", "<u4"),
                        ("set", "<u4", (WINDOW,)), ("tot", "<u4", (WINDOW,))])
MAIN_SEED = 1
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint32)


def entropy(s, t, dtype=np.float64):
    """e(s, t), left to right as the reference's C expression"""
    s = np.asarray(s, dtype)
    t = np.asarray(t, dtype)
    with np.errstate(all="ignore"):
        lt = np.log2(t)
        return (-s) * (np.log2(s) - lt) - (t - s) * (np.log2(t - s) - lt) + lt


def frame_bits(buf, off, lens, unit_log2):
    """(set, tot) of packed frames: only the len bytes of each frame count"""
    n = len(lens)
    st = np.zeros(n, np.uint32)
    for j in range(n):
        o = int(off[j]) << unit_log2
        st[j] = _POP8[buf[o:o + int(lens[j])]].sum()
    return st, (8 * lens.astype(np.uint32)).astype(np.uint32)


def pack(frames, unit_log2=6, pad=0xFF):
    """frames at off << unit_log2, every byte that is not a frame's set to
    `pad` (a counted pad byte shows), 16 spare bytes at the end"""
    unit = 1 << unit_log2
    offs, pos = [], 0
    for f in frames:
        offs.append(pos // unit)
        pos += (len(f) + unit - 1) // unit * unit   # (an empty frame takes no slot)
    buf = np.full(pos + 16, pad, np.uint8)
    for o, f in zip(offs, frames):
        buf[o * unit:o * unit + len(f)] = np.frombuffer(f, np.uint8)
    return buf, np.array(offs, np.uint32), np.array([len(f) for f in frames], np.uint16)


def density_frame(rng, nbytes, p):
    """nbytes bytes whose bits are 1 with probability p"""
    if nbytes == 0:
        return b""
    return np.packbits(rng.random(8 * nbytes) < p).tobytes()


def main_burst(seed=MAIN_SEED, n=1300):
    """the tests' main burst: 64-B frames, bit density 0.5; alternating 0.15 /
    0.85 on frames 300-699; frame 1000 all ones"""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(n):
        p = 0.5
        if 300 <= j < 700:
            p = 0.15 if (j & 1) == 0 else 0.85
        out.append(b"\xff" * 64 if j == 1000 else density_frame(rng, 64, p))
    return out


class Model:
    """the detector's state as the history of every (set, tot) seen"""

    def __init__(self):
        self.set = np.zeros(0, np.uint32)
        self.tot = np.zeros(0, np.uint32)
        self.flag = 0

    @property
    def frames_seen(self):
        return len(self.set)

    def state(self):
        """the rxg_ddos_state this history amounts to"""
        st = np.zeros(1, STATE_DTYPE)
        g = self.frames_seen
        st["frames_seen"] = g
        st["flag"] = self.flag
        for k in range(max(0, g - WINDOW), g):
            st["set"][0][k % WINDOW] = self.set[k]
            st["tot"][0][k % WINDOW] = self.tot[k]
        return st

    def run(self, st, tt, thresh=1200.0, dtype=np.float64):
        """one burst of per-frame (set, tot): dict of per-frame D, flags, S, T,
        tol and the summary; the state advances"""
        n = len(st)
        g0 = self.frames_seen
        hs = np.concatenate([self.set, np.asarray(st, np.uint32)])
        ht = np.concatenate([self.tot, np.asarray(tt, np.uint32)])
        und = (hs == 0) | (hs >= ht)
        e = np.where(und, 0, entropy(np.where(und, 1, hs), np.where(und, 2, ht), dtype)).astype(dtype)
        tl = np.where(ht > 0, ht.astype(np.float64) * np.log2(np.maximum(ht, 1).astype(np.float64)), 0.0)
        D = np.full(n, np.nan, dtype)
        S = np.zeros(n, np.uint32)
        T = np.zeros(n, np.uint32)
        tol = np.full(n, np.nan)
        flags = np.zeros(n, np.uint8)
        flag = self.flag
        summ = dict(alarm_frames=0, first_alarm=NO_ALARM, rises=0, falls=0, undef_frames=0,
                    last_stat=np.nan, last_set=0, last_tot=0)
        for j in range(n):
            g = g0 + j
            if g < WINDOW:
                flags[j] = WARMUP
                continue
            w = slice(g - WINDOW + 1, g + 1)
            S[j] = int(hs[w].astype(np.uint64).sum()) & 0xFFFFFFFF
            T[j] = int(ht[w].astype(np.uint64).sum()) & 0xFFFFFFFF
            alarm = 0
            if und[w].any():
                flags[j] = UNDEF
                summ["undef_frames"] += 1
            else:
                D[j] = e[w].sum(dtype=dtype) - entropy(S[j], T[j], dtype)
                tol[j] = 512.0 * 2.0 ** -52 * (tl[w].sum() + float(T[j]) * np.log2(float(T[j])))
                if thresh < D[j]:
                    alarm = 1
                    flags[j] = ALARM
                    summ["alarm_frames"] += 1
                    if summ["first_alarm"] == NO_ALARM:
                        summ["first_alarm"] = j
            if alarm and not flag:
                flags[j] |= RISE
                summ["rises"] += 1
            if flag and not alarm:
                flags[j] |= FALL
                summ["falls"] += 1
            flag = alarm
            summ["last_stat"], summ["last_set"], summ["last_tot"] = float(D[j]), int(S[j]), int(T[j])
        self.set, self.tot, self.flag = hs, ht, flag
        summ["flag"] = flag
        summ["frames_seen"] = self.frames_seen
        return dict(D=D, S=S, T=T, tol=tol, flags=flags, summary=summ)


def margin_ok(res, thresh):
    """no checked, defined frame within 2 tol of the threshold: the flags are
    then decided the same way by any D inside the tolerance"""
    ok = ~np.isnan(res["D"])
    return bool(np.all(np.abs(res["D"][ok].astype(np.float64) - thresh) > 2 * res["tol"][ok]))


def events(flags):
    """[(frame, 'rise' | 'fall')] of a burst's flags"""
    return [(int(j), "rise" if flags[j] & RISE else "fall")
            for j in np.nonzero(flags & (RISE | FALL))[0]]


def check_summary(got, want):
    """a DDOS_SUMMARY_DTYPE scalar against the model's summary dict: every
    field exact but last_stat (the caller compares it within tol)"""
    for k in ("frames_seen", "alarm_frames", "first_alarm", "rises", "falls", "undef_frames", "flag",
              "last_set", "last_tot"):
        assert int(got[k]) == int(want[k]), (k, int(got[k]), int(want[k]))
    assert np.isnan(got["last_stat"]) == np.isnan(want["last_stat"])


SOCK_L = "192.168.100.77"
SOCK_PORT = 8889


def socket_bursts(seed=3, sizes=(200, 150, 300, 400)):
    """the socket tests' session: bursts of 256-B UDP frames to SOCK_L:SOCK_PORT
    (every 7th to a port nobody listens on), payload bit density 0.5 but
    alternating 0.15 / 0.85 in the third burst, so that the alarm rises during
    the second burst, falls in the third and rises again in the fourth"""
    import frames as F
    rng = np.random.default_rng(seed)
    out, k = [], 0
    for b, n in enumerate(sizes):
        fr = []
        for _ in range(n):
            p = 0.5 if b != 2 else (0.15 if (k & 1) == 0 else 0.85)
            port = SOCK_PORT if k % 7 else 9
            fr.append(F.udp_frame("10.0.%d.%d" % (k >> 8 & 255, k & 255), 5000 + (k & 1023), SOCK_L, port,
                                  density_frame(rng, 214, p)))
            k += 1
        out.append(fr)
    return out


def frames_bits(frames):
    """(set, tot) of a list of frames"""
    st = np.array([int(_POP8[np.frombuffer(f, np.uint8)].sum()) for f in frames], np.uint32)
    return st, np.array([8 * len(f) for f in frames], np.uint32)
