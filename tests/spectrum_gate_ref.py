"""The spectrum's update gate in plain Python integers (pebblegpu_set_spectrum_updates; SignalSpectrum::unprocessed / ::zoomed and
setUpdatesPerSec, application/signalspectrum.cpp:63-135, with the wall clock replaced by the stream's sample clock).

Frames are numbered from the stream's first, across calls.  The frame that starts the timer gets no spectrum; after that frame f
gets one iff (f - f_last) * frame_len * 1000 // rate >= period_ms, and then becomes f_last."""

EVERY_FRAME = -1


class GateTimer:
    def __init__(self, frame_len, rate):
        self.frame_len, self.rate = int(frame_len), int(rate)
        self.updates = EVERY_FRAME
        self.period_ms = 100      # the reference's default, 10 per second
        self.started = False
        self.f_last = 0
        self.next = 0             # number of the next frame

    def set_updates(self, updates_per_sec):
        self.updates = int(updates_per_sec)
        if self.updates > 0:
            self.period_ms = 1000 // self.updates   # m_spectrumTimerUpdate = 1000 / m_updatesPerSec

    def call(self, n_frames):
        """the frames of a call of n_frames that get a spectrum, relative to the call's first frame"""
        sel = []
        for i in range(n_frames):
            f = self.next + i
            if self.updates == EVERY_FRAME:
                self.started, self.f_last = True, f
                sel.append(i)
                continue
            if not self.started:            # "First time"
                self.started, self.f_last = True, f
                continue
            if self.updates == 0:
                continue
            if (f - self.f_last) * self.frame_len * 1000 // self.rate >= self.period_ms:
                self.f_last = f
                sel.append(i)
        self.next += n_frames
        return sel


def select(frame_len, rate, updates_per_sec, calls):
    """global frame numbers selected over a list of call lengths (in frames)"""
    t = GateTimer(frame_len, rate)
    t.set_updates(updates_per_sec)
    out, base = [], 0
    for n in calls:
        out += [base + i for i in t.call(n)]
        base += n
    return out


class LatestRow:
    """'the latest computed spectrum at or before frame f': what getUnprocessed() holds when the S-meter and the squelch read it"""

    def __init__(self):
        self.frames = []   # global numbers of the computed frames, ascending

    def add(self, global_frames):
        self.frames += list(global_frames)

    def at(self, f):
        """index into the list of computed frames, or None before the first"""
        k = None
        for i, g in enumerate(self.frames):
            if g <= f:
                k = i
        return k
