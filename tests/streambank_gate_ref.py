"""The stream bank's update gate in plain Python integers (pebblegpu_streambank_set_spectrum_updates): the receiver's model
(tests/spectrum_gate_ref.py) plus the one rule a bank adds -- a call WITHOUT the spectrum advances the sample clock and nothing else."""
from tests.spectrum_gate_ref import EVERY_FRAME, GateTimer  # noqa: F401  (EVERY_FRAME re-exported)


class BankGateTimer(GateTimer):
    def skip(self, n_frames):
        """a call of n_frames that did not ask for the spectrum: no frame is selected, the timer is neither started nor restarted"""
        self.next += n_frames


def select(frame_len, rate, updates_per_sec, calls):
    """per call (lengths in frames) the selected frames relative to the call's first"""
    t = BankGateTimer(frame_len, rate)
    t.set_updates(updates_per_sec)
    return [t.call(n) for n in calls]
