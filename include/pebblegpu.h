/*
 * pebblegpu.h -- C ABI of libpebblegpu: PebbleSDR's per-frame IQ receive chain on MI355X (gfx950).
 *
 * This is the drop-in boundary for ONE hot path of the reference: what Receiver::processIQData
 * (application/receiver.cpp:758-1009) runs between the device plugin's callback and the audio
 * resampler -- Mixer, Decimator, CFastFIR band-pass, Demod (AM / WFM mono / SSB-CW-DIG pass-through)
 * and the SignalSpectrum FFT.  Plain pointers and sizes only; no C++/Qt/torch types cross it.
 * Every entry point names the reference interface it replaces (paths relative to the reference).
 *
 * Conventions
 *   - host complex buffers are interleaved (re, im) doubles == CPX = std::complex<double>
 *     (pebblelib/cpx.h:96); device complex buffers are interleaved (re, im) floats ("float2").
 *   - all functions return PEBBLEGPU_OK (0) or a negative pebblegpu_status; nothing throws across
 *     the ABI; pebblegpu_last_error() returns text for the calling thread's last failure.
 *   - process_* calls are single-caller per handle (the reference calls processIQData from one
 *     consumer thread, pebblelib/producerconsumer.cpp:101-109); setters may be called from another
 *     thread and take effect at the next process call (= frame boundary).
 *   - ASYNCHRONY: pebblegpu_receiver_process / _process_raw and pebblegpu_streambank_process / _process_raw only QUEUE their kernels on
 *     streams private to the handle and return.  The device buffers behind pebblegpu_receiver_audio / _spectrum /
 *     _signal_strength and pebblegpu_streambank_filtered / _spectrum hold the call's results, and the call's INPUT buffer
 *     may be overwritten, only after pebblegpu_receiver_synchronize / pebblegpu_streambank_synchronize (or any of
 *     pebblegpu_memcpy_h2d / _d2h / pebblegpu_device_synchronize, which wait for all work queued on the device first).
 *     A host that touches those buffers with its own HIP calls must synchronise itself.  Calls on one handle execute in
 *     the order they were made.  A receiver without a display transform runs a call as two overlapping stages on two streams
 *     (two-stage calls) and bounds how far the host may run ahead: such a call returns once the call three
 *     before it has completed.  The host-buffer entry points (pebblegpu_process_iq and every stand-alone step) return
 *     with their results complete.
 *   - the library owns every device buffer it returns; host pointers returned by *_result() stay
 *     valid until the next process call on the same handle (ProcessStep ownership rule,
 *     application/processstep.cpp:12-20).  Inputs are never modified (receiver.cpp:747-755).
 */
#ifndef PEBBLEGPU_H
#define PEBBLEGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PEBBLEGPU_ABI_VERSION 1

typedef enum {
    PEBBLEGPU_OK = 0,
    PEBBLEGPU_E_INVALID = -1,      /* bad argument / bad handle */
    PEBBLEGPU_E_NO_DEVICE = -2,    /* no HIP device: the library never falls back to the CPU */
    PEBBLEGPU_E_HIP = -3,          /* HIP runtime error, see pebblegpu_last_error() */
    PEBBLEGPU_E_FILTER_PARAM = -4, /* CFastFIR "Filter Parameter error": previous taps stay active
                                      (pebblelib/fastfir.cpp:208-216) */
    PEBBLEGPU_E_SIZE = -5,         /* sample count not a whole number of super-frames / too large */
    PEBBLEGPU_E_UNSUPPORTED = -6   /* mode or size outside what this build implements */
} pebblegpu_status;

/* DeviceInterface::DemodMode numeric values, pebblelib/device_interfaces.h:124-138 (a Qt shim maps 1:1) */
typedef enum {
    PEBBLEGPU_DM_AM = 0, PEBBLEGPU_DM_SAM, PEBBLEGPU_DM_FMN, PEBBLEGPU_DM_FMM, PEBBLEGPU_DM_FMS,
    PEBBLEGPU_DM_DSB, PEBBLEGPU_DM_LSB, PEBBLEGPU_DM_USB, PEBBLEGPU_DM_CWL, PEBBLEGPU_DM_CWU,
    PEBBLEGPU_DM_DIGL, PEBBLEGPU_DM_DIGU, PEBBLEGPU_DM_NONE
} pebblegpu_demod_mode;

const char *pebblegpu_last_error(void);
int pebblegpu_abi_version(void);
/* number of HIP devices visible (0 => every create() fails with PEBBLEGPU_E_NO_DEVICE) */
int pebblegpu_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * Device memory + stream plumbing (so a host needs no other GPU library to feed the chain)
 * ---------------------------------------------------------------------------------------------- */
int pebblegpu_malloc(int device, size_t bytes, void **dptr);
int pebblegpu_free(int device, void *dptr);
/* both copies first wait for all work queued on the device (the library's private streams included), then copy and block */
int pebblegpu_memcpy_h2d(int device, void *dst, const void *src, size_t bytes);
int pebblegpu_memcpy_d2h(int device, void *dst, const void *src, size_t bytes);
int pebblegpu_memset(int device, void *dst, int value, size_t bytes);
int pebblegpu_device_synchronize(int device);
/* Streaming-copy probe (read + write GB/s of a plain device copy with 16- or 8-byte lanes): the measured HBM ceiling
 * the bench quotes next to the 8 TB/s datasheet peak. */
int pebblegpu_probe_copy_gbps(int device, int lane_bytes, size_t bytes, int iters, float *gbps);
/* Diagnostic: the bytes of device memory and of pinned host memory that THIS library holds in THIS process right now, over all
 * devices and handles (what pebblegpu_malloc handed to the host is the host's and is not counted).  Either pointer may be NULL.
 * Every handle's destroy brings both back to what they were before its create: a leak check that does not read the device's free
 * memory, which other processes on the same device change. */
int pebblegpu_live_bytes(uint64_t *device, uint64_t *pinned);
/* Ingest on the device: DeviceInterfaceBase::normalizeIQ (pebblelib/deviceinterfacebase.cpp:648-838) and
 * WavFile::ReadSamples' PCM16 scaling (wavfile.cpp:299-300).  d_src holds n_samples raw IQ pairs, d_dst receives float2.
 * gain = m_userIQGain * m_normalizeIQGain; iq_order = DeviceInterface::IQOrder (device_interfaces.h:140-145). */
typedef enum {
    PEBBLEGPU_IQ_S8 = 0,    /* CPX8  (HackRF):  v / 128 */
    PEBBLEGPU_IQ_U8 = 1,    /* CPXU8 (RTL2832): (v - 128) / 128 */
    PEBBLEGPU_IQ_S16 = 2,   /* CPX16: v / 32768 */
    PEBBLEGPU_IQ_F32 = 3,   /* CPXFLOAT */
    PEBBLEGPU_IQ_WAV16 = 4  /* 16-bit PCM stereo WAV: v / 32767 */
} pebblegpu_iq_format;
typedef enum { PEBBLEGPU_IQO_IQ = 0, PEBBLEGPU_IQO_QI, PEBBLEGPU_IQO_IONLY, PEBBLEGPU_IQO_QONLY } pebblegpu_iq_order;
int pebblegpu_normalize_iq(int device, int format, int iq_order, double gain, const void *d_src, uint64_t n_samples, void *d_dst);

/* ------------------------------------------------------------------------------------------------
 * Receiver bank: C tuned channels over one shared wideband stream, or C independent streams.
 * Replaces Receiver::turnPowerOn's step construction (receiver.cpp:154-264) and
 * Receiver::processIQData's DSP (receiver.cpp:826-987).
 * ---------------------------------------------------------------------------------------------- */
typedef struct pebblegpu_receiver pebblegpu_receiver;

typedef struct {
    uint32_t struct_size;        /* = sizeof(pebblegpu_config) */
    int32_t device;              /* HIP device ordinal */
    double sample_rate;          /* Fs of the device stream, Hz (Key_SampleRate, receiver.cpp:149) */
    uint32_t frames_per_buffer;  /* reference N: settings.cpp:57 default 2048; spectrum window length */
    uint32_t n_channels;         /* C */
    uint32_t shared_input;       /* 1: all channels read stream 0; 0: channel c reads stream c */
    uint32_t wfm;                /* 0: narrow branch (protect 30 kHz + FastFIR, receiver.cpp:903-993)
                                    1: WFM branch (protect 200 kHz, no band-pass, receiver.cpp:854-901) */
    uint32_t spectrum_bins;      /* 0: no spectrum; else FFT size (settings.cpp:59 default 4096) */
    uint32_t fastfir_fft;        /* 0 -> 2048 (fastfir.cpp:65); 2048, 4096 or 8192 */
    uint32_t fastfir_taps;       /* 0 -> 1025 (fastfir.cpp:66); 2 .. fastfir_fft/2 + 1, else PEBBLEGPU_E_INVALID: the overlap
                                    (taps-1) may not exceed the block (fft - overlap) */
    uint32_t max_superframes;    /* capacity of one process call, in super-frames (>=1) */
    uint32_t audio_rate;         /* 0: audio stays at the demod rate (resampRate == 1, receiver.cpp:1002-1003); else
                                    Key_AudioOutputSampleRate (receiver.cpp:203, default 11025): the audio buffer is
                                    CFractResampler::Resample(n, demodRate / audio_rate, ...) of the demodulated frames
                                    (receiver.cpp:994-1001, pebblelib/fractresampler.cpp:149-195).  Rates above the demod rate
                                    (upsampling) are accepted: the audio rows hold n * audio_rate / demodRate + frames + 8 samples */
    uint32_t hires_bins;         /* 0: no zoomed spectrum (m_useHiRes off); else the bin count of SignalSpectrum::zoomed
                                    (application/signalspectrum.cpp:89-113; settings.cpp:61 default 2048): fftSpectrum, BlackmanHarris
                                    over frames_per_buffer samples, of every DECIMATED frame of every channel -- m_sampleBuf at the
                                    demodulator rate, after the gain restore on the narrow branch (receiver.cpp:884, 942) */
    uint32_t reserved[3];
} pebblegpu_config;

int pebblegpu_receiver_create(const pebblegpu_config *cfg, pebblegpu_receiver **out);
int pebblegpu_receiver_destroy(pebblegpu_receiver *rx);

/* What buildDecimationChain (pebblelib/decimator.cpp:64-149) produced for this bank. */
typedef struct {
    double demod_rate;           /* achieved rate (float in the reference) */
    uint32_t demod_rate_int;     /* the int the Receiver stores and designs filters with (receiver.h:165-166) */
    uint32_t dec_by2_stages;     /* Decimator::decBy2Stages() */
    uint32_t total_decimation;   /* D */
    uint32_t chain_len;          /* merged stages; 0 where no design fits the rate (below 75 kHz narrow, below 500 kHz WFM): the
                                    reference's "No decimation" (decimator.cpp:155-160), D = 1, the demodulator at the input rate */
    uint32_t stage_taps[16];     /* 0 => CIC3 */
    uint32_t stage_stride[16];
    uint64_t superframe;         /* input samples per super-frame = D * frames_per_buffer */
    uint32_t n_streams;
    uint32_t spectrum_bins;      /* after the reference's [2048, 65535] clamp (fft.cpp:72-79) */
} pebblegpu_info;
int pebblegpu_receiver_info(const pebblegpu_receiver *rx, pebblegpu_info *info);

/* Receiver::mixerChanged -> Mixer::setFrequency (receiver.cpp:709-716, mixer.cpp:25-40): negated
 * frequency, oscillator phase AND amplitude reset to (1,0). */
int pebblegpu_set_mixer_freq(pebblegpu_receiver *rx, uint32_t channel, double freq_hz);
/* Receiver::filterChanged (receiver.cpp:658-664): BandPassFilter::setBandPass -> CFastFIR::SetupParameters
 * (lo, hi, offset 0, demod rate) and, for AM channels, Demod_AM::setBandwidth(hi - lo). */
int pebblegpu_set_bandpass(pebblegpu_receiver *rx, uint32_t channel, double lo_hz, double hi_hz);
/* Receiver::demodModeChanged -> Demod::setDemodMode (receiver.cpp:640-655).  Narrow banks accept AM, SAM, FMN and
 * every pass-through mode (DSB/LSB/USB/CWL/CWU/DIGL/DIGU/NONE); WFM banks accept FMM (mono) and FMS.
 * FMS is Demod_WFM::processDataStereo (demod_wfm.cpp:255-365): the discriminator output WITHOUT processDataMono's 75 kHz
 * pre-filter, low-passed, de-emphasised and notched; while the pilot PLL (processPilotPll, :390-430) reports lock at the end of a
 * block of frames_per_buffer samples that block is demultiplexed (left - right = 2 raw sin(2 phase)), otherwise it carries the same
 * signal in both channels.  The PLL's phase detector (:792-821) is discontinuous at the loop's operating point and the lock is lost
 * within the first blocks on every input it has been tried on (pinned on the oracle's line-by-line restatement with clean, noisy,
 * weak and absent pilots at the demodulator rates the receiver runs, tests/test_oracle_pins.py -- other inputs: parity unpinned);
 * the library runs the loop, serially per channel, until the first block that ends without lock and treats the stream as mono from
 * there (the lock average would need seconds of a quiet detector to come back).  The RDS branch of the same function (:296-357:
 * m_RdsDownConvert, the 2400 Hz low-pass, processRdsPll, the biphase matched filter, the bit-rate resonator and slicer,
 * processNewRdsBit's block synchroniser with its burst corrector) runs for every dmFMS channel, in double on the device; its groups are
 * read through pebblegpu_receiver_rds_groups.  The frame of a dmFMS bank (frames_per_buffer at the demodulator rate) must be a multiple
 * of the RDS down-converter's decimation D (8 up to 312.5 kHz of demodulator rate, 16 from 384 kHz on) and leave every decimate-by-2
 * stage j at least 2 (T_j - 1) samples (frame >> j; more than 18 for the fixed 11-tap stage): below that the reference's in-place
 * DecBy2 keeps outputs where its history should be (see pebblegpu_downconvert_process) and a frame-by-frame receiver would not be the
 * reference.  The shortest frames: 272 at 256 kHz (15, 19, 35 taps), 800 at 384 kHz (11, 15, 23, 51).  A handle whose frame does not
 * fit REFUSES THE MODE CHANGE with PEBBLEGPU_E_SIZE and the rule in the text: the channel stays dmFMM, nothing is queued, nothing
 * about the next call changes, and the handle goes on.  Not reproduced: what the GUI makes of a group (rdsdecode.cpp). */
int pebblegpu_set_demod_mode(pebblegpu_receiver *rx, uint32_t channel, int mode);
/* tRDS_GROUPS (application/demod/rbdsconstants.h) */
typedef struct pebblegpu_rds_group { uint16_t block_a, block_b, block_c, block_d; } pebblegpu_rds_group;
/* int Demod_WFM::getNextRdsGroupData(tRDS_GROUPS *), demod_wfm.h:39, as its one caller uses it (Demod::fmStereo, demod.cpp:196-226:
 * ONE call behind every processDataStereo, i.e. per frame of frames_per_buffer demodulator samples): the groups that caller would
 * have taken from m_RdsGroupQueue (RDS_Q_SIZE 100, cleared and stuffed with a zero group after BLOCK_ERROR_LIMIT bad blocks) over the
 * frames processed since the last call of this function, oldest first, and for each the function's return value -- changed[i] != 0:
 * the group differs from the one delivered before it (only those reach the reference's text decoder, and only when block_a != 0).
 * Waits for the receiver's queued work.  *n: entries written (<= cap; the rest stays for the next call). */
int pebblegpu_receiver_rds_groups(pebblegpu_receiver *rx, uint32_t channel, pebblegpu_rds_group *groups, uint8_t *changed, uint32_t cap,
                                  uint32_t *n);
/* int Demod_WFM::getStereoLock(int *pPilotLock), demod_wfm.h:40 (demod_wfm.cpp:436-447): *pilot_lock = m_PilotLocked after the last
 * frame of the channel (0 before its first dmFMS frame), *changed != 0 when that differs from what the previous call of this function
 * reported (the first call reports a change: m_LastPilotLocked starts as the opposite).  Waits for the receiver's queued work. */
int pebblegpu_receiver_stereo_lock(pebblegpu_receiver *rx, uint32_t channel, int *pilot_lock, int *changed);
/* The digital-modem hook between the noise filter and the AGC (application/receiver.cpp:977-980), with the Morse decoder
 * (plugins/MorseDigitalModem, its default Goertzel path) per channel of a narrow receiver: Decimator to about 8 kHz
 * (buildDecimationChain(demodRate, 1000, 8000)), a Goertzel bin of N samples at +-1000 Hz, GoertzelOOK's TH_PEAK threshold and
 * Morse::stateMachine, on the device behind every call.  The library emits the reference's token per completed character (a leading 1,
 * then 1 per dash and 0 per dot, at most 8 elements: MorseCode::tokenizeDotDash, morsecode.cpp:160-185) and a word-space event;
 * the application renders text with MorseCode::tokenLookup ("*" when it returns nothing).  See DESIGN.md section 3. */
typedef struct pebblegpu_morse_event {
    uint64_t sample;  /* modem-rate samples since the modem was enabled, up to the one whose Goertzel result decided the event */
    uint32_t token;   /* kind PEBBLEGPU_MORSE_CHAR: the token; PEBBLEGPU_MORSE_WORD_SPACE: 0 */
    uint32_t kind;
} pebblegpu_morse_event;
#define PEBBLEGPU_MORSE_CHAR 0u
#define PEBBLEGPU_MORSE_WORD_SPACE 1u
/* what Morse::refreshOutput shows (morse.cpp:477-500): the WPM estimate (m_wpmSpeedCurrent; "?? est" when a flag is set), the
 * out-of-range flags, the modem rate and N (Goertzel samples per result) */
typedef struct pebblegpu_morse_report {
    int32_t wpm, above_range, below_range;
    uint32_t modem_rate, samples_per_result;
} pebblegpu_morse_report;
/* Receiver::setDigitalModem("Morse") + Morse::setSampleRate(m_demodSampleRate, m_demodFrames) (on != 0, also on a channel whose modem is
 * already on): a fresh decoder in dmCWL whatever the channel's mode (morse.cpp:181; later pebblegpu_set_demod_mode calls are forwarded,
 * receiver.cpp:653-654), starting from the channel's current WPM estimate (20 the first time); events decided before stay readable.
 * on == 0 drops the decoder's state and its unread events.  Channels in dmNONE and calls closed by
 * the squelch of a one-channel receiver leave the modem untouched.  Refused (PEBBLEGPU_E_UNSUPPORTED) by WFM receivers and together
 * with a bank's per-channel squelch (by whichever of the two setters comes second).  Waits for the channel's queued modem work. */
int pebblegpu_set_morse(pebblegpu_receiver *rx, uint32_t channel, int on);
/* the channel's events since the last read, oldest first (*n <= cap; the rest stays).  None is lost however many calls run between
 * two reads.  Waits for the receiver's queued modem work. */
int pebblegpu_receiver_morse_events(pebblegpu_receiver *rx, uint32_t channel, pebblegpu_morse_event *ev, uint32_t cap, uint32_t *n);
int pebblegpu_receiver_morse_status(pebblegpu_receiver *rx, uint32_t channel, pebblegpu_morse_report *st);
/* AGC::setAgcMode(mode, threshold) (application/agc.cpp:53-82; Receiver::agcModeChanged/agcThresholdChanged).
 * agc_mode: the reference's AgcMode values.  With PEBBLEGPU_AGC_OFF the threshold is a manual gain slider in dB
 * (amplitude 10^((threshold/5)/20), integer division as written, agc.cpp:239-246; the constructor's OFF/1 is unit
 * gain); otherwise it is the knee (0..120, negated inside).  Narrow banks only: the WFM branch has no AGC step. */
typedef enum pebblegpu_agc_mode {
    PEBBLEGPU_AGC_OFF = 0, PEBBLEGPU_AGC_FAST = 1, PEBBLEGPU_AGC_MED = 2, PEBBLEGPU_AGC_SLOW = 3, PEBBLEGPU_AGC_LONG = 4
} pebblegpu_agc_mode;
int pebblegpu_set_agc(pebblegpu_receiver *rx, uint32_t channel, int agc_mode, int threshold);

/* Batched device path.  d_iq: n_streams x n_samples float2 (stream-major, [stream][time]); n_samples must be
 * k * superframe (k <= max_superframes).  Outputs (library-owned device buffers, valid until the next call):
 *   audio    [channel][k * frames_per_buffer] float2  (re = left, im = right, receiver.cpp:1029); with audio_rate
 *            set, the resampled audio instead: the count pebblegpu_receiver_audio reports (same for all channels)
 *   spectrum [stream][n_samples / frames_per_buffer][bins] float, dB amplitude, -f..+f (fft.cpp:395) */
/* Frames shorter than a stage's tap count: the library streams with exact history for any n_samples that is a whole number of
 * super-frames.  The reference, fed 2048-sample frames at >= 20 Msps, degrades such stages to unfiltered sample dropping and
 * refills their history from indeterminate memory (pebblelib/decimator.cpp:602-625); that fallback is NOT reproduced (DESIGN.md
 * section 4, tests/test_parity_gpu.py::test_decimator_short_frames_stream_exactly).  Queues and returns: see ASYNCHRONY above. */
int pebblegpu_receiver_process(pebblegpu_receiver *rx, const void *d_iq, uint64_t n_samples);
/* The same call fed with the device's own sample format (what ProducerConsumer hands normalizeIQ,
 * deviceinterfacebase.cpp:648-838): d_raw holds n_streams x n_samples raw IQ pairs, stream-major, in `format`
 * (pebblegpu_iq_format) and `iq_order`, scaled by the format's constant and `gain` (gain 0 is silence).  Results equal
 * pebblegpu_receiver_process on the same samples converted on the host with the same constants, bit for bit, whichever way the call goes:
 *   converted in the loads -- one stream, one channel beside the 8192-bin display transform, a first decimator stage hb11 x S (the
 *     headline shape among them), no conditioner, generator, squelch value or per-kernel profiling on, and no oscillator inside its
 *     amplitude transient (the first call of a handle and the call behind a retune are): the display transform and the first stage
 *     read the raw pairs themselves and no float2 copy of the stream exists.  The recording ring and the RAW_IQ tap read the raw pairs too;
 *   staged -- every other call: k_normalize_iq converts all streams into a library-owned float2 buffer on the library's stream (no host
 *     synchronisation) and the call goes on from there.
 * pebblegpu_receiver_kernel_name(rx, 6) says which it was.  d_raw must be aligned to PEBBLEGPU_RAW_ALIGN bytes on either route (the
 * converting loads read 8, 16 and 32 bytes at a time), which every allocation and every whole super-frame inside one is.  Refused
 * before anything is queued, leaving the handle usable: a null or misaligned d_raw, an unknown format or IQ order
 * (PEBBLEGPU_E_INVALID); more samples than the capacity or not whole super-frames (PEBBLEGPU_E_SIZE).  pebblegpu_receiver_process_ingested
 * and the multibank's raw calls make the same call per slot or shard (their buffers are allocations of the library's own) and refuse
 * the same. */
int pebblegpu_receiver_process_raw(pebblegpu_receiver *rx, int format, int iq_order, double gain, const void *d_raw, uint64_t n_samples);
/* Host ingest through the library's own pinned buffers (the device plugins' producer side, e.g. the HackRF callback that fills
 * the producer/consumer ring, plugins/HackRFDevice/hackrfdevice.cpp:533-566, writes its raw samples straight into one): two slots,
 * so that the upload of one batch crosses PCIe on a copy stream while the call on the other batch computes.
 *   acquire  -- the slot's pinned host buffer of at least `bytes` (grown on demand); blocks until the last call that read the slot
 *               is over, then the host may fill it.  The pointer stays valid until the next acquire of that slot with a larger size.
 *   submit   -- queues the upload of the first `bytes` of the slot (returns at once; the host must not touch the slot until it
 *               has acquired it again);
 *   process_ingested -- pebblegpu_receiver_process_raw on the uploaded samples, ordered behind the upload on the device (no host
 *               synchronisation).  n_streams x n_samples pairs of `format` must have been submitted.
 * Steady state of a producer: acquire(s), fill, submit(s), process_ingested(s), s ^= 1 -- with the audio of the previous call read
 * in between.  The PCIe link bounds this path (2 bytes per sample for HackRF/RTL pairs); DESIGN.md section 5 has the measured rates. */
int pebblegpu_receiver_ingest_acquire(pebblegpu_receiver *rx, uint32_t slot, uint64_t bytes, void **host_ptr);
int pebblegpu_receiver_ingest_submit(pebblegpu_receiver *rx, uint32_t slot, uint64_t bytes);
int pebblegpu_receiver_process_ingested(pebblegpu_receiver *rx, uint32_t slot, int format, int iq_order, double gain, uint64_t n_samples);
/* returns channel 0's row; channel c starts *pitch_samples float2 further per channel */
const void *pebblegpu_receiver_audio(const pebblegpu_receiver *rx, uint64_t *samples_per_channel, uint64_t *pitch_samples);
const void *pebblegpu_receiver_spectrum(const pebblegpu_receiver *rx, uint64_t *frames_per_stream);
/* the zoomed (hi-res) spectra of the last call: [channel][frames_per_channel][bins] float dB, -f..+f at the demodulator rate */
const void *pebblegpu_receiver_zoom_spectrum(const pebblegpu_receiver *rx, uint64_t *frames_per_channel, uint32_t *bins);
/* SignalSpectrum::setUpdatesPerSec (application/signalspectrum.cpp:124-135; SpectrumWidget::updatesPerSecChanged calls it): the gate
 * in front of SignalSpectrum::unprocessed and ::zoomed (:63-113).  Open by default (PEBBLEGPU_SPECTRUM_EVERY_FRAME: every frame gets a
 * spectrum, as before this setter existed).  0: no unprocessed and no zoomed spectrum is computed (m_updatesPerSec == 0).  A rate > 0:
 * the reference's rule with its wall clock replaced by the stream's own sample clock, so that the selection does not depend on how fast
 * or in what call sizes the host feeds the library: period_ms = 1000 / updates_per_sec (integer division); frames are numbered from the
 * handle's creation, across calls; the frame that starts the timer gets no spectrum; after that frame f gets one iff
 * (f - f_last) * frames_per_buffer * 1000 / sample_rate >= period_ms (integer arithmetic, the rate in whole Hz) and then becomes f_last.
 * Changing the rate changes the period only, the timer runs on: coming from the default it counts from the last frame of the previous
 * call (or is started by the first frame), coming from 0 it has kept its f_last.  The zoomed spectrum has a timer of its own with the
 * same period over the decimated frames of each channel (frames_per_buffer * 1000 / info.demod_rate_int per frame).
 * With a gate set:
 *   - the frame list is worked out on the host before anything is queued (no read-back, no synchronisation);
 *   - pebblegpu_receiver_spectrum / _zoom_spectrum return the COMPUTED rows only, compact: [stream][n_selected][bins], the frame count
 *     they report is n_selected (possibly 0); pebblegpu_receiver_spectrum_frames says which frames they are; the map functions and the
 *     S-meter index these rows (after a call that made no unprocessed spectrum pebblegpu_receiver_map_spectrum maps the latest one made
 *     before it, as frame 0: what the display still shows); a frame's spectrum is averaged with the previous COMPUTED frame's (m_fftAmplitude, fft.cpp:378-386),
 *     across calls;
 *   - the squelch reads avgDb of the latest computed spectrum at or before the super-frame's last raw frame, from an earlier call if
 *     need be (getUnprocessed(), receiver.cpp:891-897, 959-965); before the first spectrum the gate stays open;
 *   - audio is the same on every route. */
#define PEBBLEGPU_SPECTRUM_EVERY_FRAME (-1)
int pebblegpu_set_spectrum_updates(pebblegpu_receiver *rx, int updates_per_sec);
/* which frames of the last call got an unprocessed (zoomed != 0: a zoomed) spectrum: indices relative to the call's first frame,
 * ascending, row i of the spectrum buffer belongs to idx[i].  *n entries are written (every frame of the call without a gate);
 * PEBBLEGPU_E_SIZE when cap is too small.  Known the moment the process call returns. */
int pebblegpu_receiver_spectrum_frames(const pebblegpu_receiver *rx, int zoomed, uint32_t *idx, uint32_t cap, uint32_t *n);

/* ------------------------------------------------------------------------------------------------
 * Spectrum to display pixels: FFT::mapFFTToScreen (pebblelib/fft.cpp:400-534), the call SpectrumWidget makes for every plot and
 * every waterfall row (through SignalSpectrum::mapFFTToScreen / mapFFTZoomedToScreen, application/signalspectrum.cpp:137-167).
 * Each spectrum row of fftSize dB values becomes x_pixels plot heights in 0..y_pixels-1: bins are averaged in power where several
 * fall on one pixel (the reference's window [previous pixel's bin, this pixel's bin), and only from pixel 2 on), repeated where one
 * bin spans several pixels, -120 dB outside the spectrum.  The arithmetic is the reference's as an x86-64 build runs it (float where
 * it is float, no contraction, truncating conversions); the per-pixel power sum may be added in another order and pow / log10 are
 * the device's: an averaged pixel whose unrounded value lies within 1e-9 of an integer may come out one powerdB step away.
 * Refused before anything is queued, leaving the handle usable (PEBBLEGPU_E_INVALID): x_pixels <= 0, y_pixels <= 0,
 * max_db == min_db, a handle with no such spectrum or no call yet, a frame range beyond the last call.  Every other input the
 * reference accepts is reproduced, start_freq >= stop_freq and ranges wholly outside the spectrum included.
 * ---------------------------------------------------------------------------------------------- */
typedef struct pebblegpu_screen_map {
    uint32_t struct_size;           /* = sizeof(pebblegpu_screen_map) */
    int32_t y_pixels;               /* plot height; 255 for the waterfall colour index (spectrumwidget.cpp:1285-1293) */
    int32_t x_pixels;               /* plot width */
    double max_db, min_db;          /* dB at the top / bottom of the plot */
    int32_t start_freq, stop_freq;  /* Hz, relative to the spectrum's centre */
    uint32_t reserved[4];
} pebblegpu_screen_map;
/* Maps frames first_frame + j * frame_step (j < n_frames) of every stream of the last call's unprocessed spectrum
 * (pebblegpu_receiver_spectrum; sampleRate = the configured stream rate, fftSize = info.spectrum_bins) into the device buffer
 * d_out: int32 [stream][n_frames][x_pixels].  Queued behind the call's display transform and ahead of the next call's, on the
 * receiver's streams (default side-by-side calls and PEBBLEGPU_PIPELINE=1 alike); d_out holds the result after
 * pebblegpu_receiver_synchronize.  A display that shows one frame maps the last one; a waterfall maps a stride. */
int pebblegpu_receiver_map_spectrum(pebblegpu_receiver *rx, const pebblegpu_screen_map *map, uint32_t first_frame, uint32_t n_frames,
                                    uint32_t frame_step, int32_t *d_out);
/* The same on the zoomed spectra (pebblegpu_receiver_zoom_spectrum), per channel: int32 [channel][n_frames][x_pixels].  As
 * SignalSpectrum::mapFFTZoomedToScreen (signalspectrum.cpp:151-167): quint16 span = hiResRate * zoom, start = -span/2 - offset,
 * stop = span/2 - offset in int, hiResRate = info.demod_rate_int (the rate the zoomed transform ran at, receiver.cpp:221,644-646),
 * offset = mode_offset[channel] (host array of n_channels; NULL: all 0).  A product hiResRate * zoom of 65536 or more does not fit
 * the quint16 and the reference's conversion is undefined: as on x86-64 it is truncated to int32 and the low 16 bits are kept. */
int pebblegpu_receiver_map_zoom_spectrum(pebblegpu_receiver *rx, int32_t y_pixels, int32_t x_pixels, double max_db, double min_db, double zoom,
                                         const int32_t *mode_offset, uint32_t first_frame, uint32_t n_frames, uint32_t frame_step,
                                         int32_t *d_out);
/* Time of the last process call's kernels in ms, from HIP events on the library's stream.  which: 0 whole
 * call; 1 spectrum kernel; 2 mixer+first-decimator kernel; 3 remaining decimator stages; 4 FastFIR;
 * 5 demod.  A call whose chain runs beside its display transform records no end event of its own: which = 0
 * of such a call runs to the start event of the NEXT call on the handle (recorded behind that call's control
 * updates and, for raw input that is staged, its conversion pass), or to the pebblegpu_receiver_synchronize /
 * timing query that closes it -- back to back the sum over calls is the wall time, a single call's figure
 * includes whatever the host let pass before it queued the next one.  PEBBLEGPU_EVENTS=full (read when the
 * receiver is created) gives every call an end event of its own.
 * A receiver WITHOUT a display transform (spectrum_bins = 0) runs a call in two stages on two streams -- mixer + decimator, then
 * band-pass .. resampler -- the second beside the NEXT call's first when calls are queued back to back: which = 0 of such a call
 * runs from the end of the previous call's first stage to the end of its own second stage (its latency; back to back the calls
 * overlap, so the figures sum to more than the wall time).  PEBBLEGPU_BANK_PIPELINE=0 (read when the receiver is created) keeps
 * every call on one stream; set_profiling(rx, 1) does the same for as long as it is on. */
int pebblegpu_receiver_last_ms(const pebblegpu_receiver *rx, int which, float *ms);
/* name(s) of the kernel(s) behind group `which` (1..5) as the last process call ran them ("" when the group is empty): the
 * bench labels its per-kernel roofline lines with these.
 * which = 6 is the input route of the last process call instead: "float2" (pebblegpu_receiver_process), "raw s8" / "raw u8" /
 * "raw s16" / "raw f32" / "raw wav16" (a raw call whose first kernels converted that format in their own loads; the stream bank's
 * tags), "k_normalize_iq" (a raw call staged through the conversion pass), "" before the first call.  A refused call leaves it alone. */
const char *pebblegpu_receiver_kernel_name(const pebblegpu_receiver *rx, int which);
/* which 0 and 1 are always available (two event records per call, three with a display transform; 1 reads 0 without one).  The per-kernel splits 2..5 need four more
 * records, each a ~5 us bubble in the stream, so they are recorded only after set_profiling(rx, 1). */
int pebblegpu_receiver_set_profiling(pebblegpu_receiver *rx, int per_kernel);
/* the same, averaged over the last `last_k` process calls (the library keeps events for 64): lets a caller queue calls
 * back to back without a host sync per call and read the kernel times afterwards */
int pebblegpu_receiver_mean_ms(const pebblegpu_receiver *rx, int which, uint32_t last_k, float *ms);
/* Input conditioners, applied in the reference's order to a copy of the stream before the spectrum and the mixer
 * (receiver.cpp:814-823); all default-off.  flags: PEBBLEGPU_COND_* or'ed.  DC: DCRemoval (CIir high-pass 10 Hz, Q
 * 0.7071, dcremoval.cpp:3-19); IQBALANCE: IQBalance::ProcessBlock with setGainFactor/setPhaseFactor values
 * (iqbalance.cpp:65-86); NB1/NB2: NoiseBlanker::ProcessBlock/ProcessBlock2 (noiseblanker.cpp:45-97; switching one on
 * resets its averages as setNbEnabled does).  These are serial-in-time algorithms: the library runs one lane per stream
 * (per frame for IQBALANCE), so they parallelise over banks of streams, not within one.  Batched device path only.
 * A blanker is reset on the off -> on TRANSITION of its flag only: a setter call with the flag already on (another gain, say) leaves its
 * averages, NB1's spike count and delay line where the stream left them.  (The reference's setNbEnabled(true) resets whenever it is
 * called; its UI calls it on a toggle.)  IQBALANCE is switched by its flag alone: iq_gain and iq_phase are applied as given, a negative
 * gain included (the reference multiplies by it).  IQBalance restarts its adaptive terms every frames_per_buffer samples.
 * PEBBLEGPU_E_INVALID, nothing changed and the handle usable afterwards: a NULL handle, a stream out of range, flags outside 0..15, a
 * non-finite iq_gain or iq_phase.
 *
 * pebblegpu_receiver_conditioned(rx, &samples_per_stream, &pitch_samples): a device pointer to float2 [stream][pitch], the conditioned
 * rows the LAST call's spectrum and mixer read; valid after pebblegpu_receiver_synchronize until the next call.  NULL and both outputs 0
 * when the last call conditioned nothing: no flag set on any stream, a refused call, pebblegpu_process_iq.  It hands out what the call
 * made anyway: no launch, copy or allocation of its own. */
enum { PEBBLEGPU_COND_DC = 1, PEBBLEGPU_COND_IQBALANCE = 2, PEBBLEGPU_COND_NB1 = 4, PEBBLEGPU_COND_NB2 = 8 };
int pebblegpu_set_conditioners(pebblegpu_receiver *rx, uint32_t stream, int flags, double iq_gain, double iq_phase);
const void *pebblegpu_receiver_conditioned(const pebblegpu_receiver *rx, uint64_t *samples_per_stream, uint64_t *pitch_samples);
/* NoiseFilter (ANF, 45-tap leaky LMS on a 64-sample delay, noisefilter.cpp:31-88) on a narrow channel, between the
 * band-pass and the AGC (receiver.cpp:974) */
int pebblegpu_set_noise_filter(pebblegpu_receiver *rx, uint32_t channel, int on);
/* S-meter: SignalStrength::fdEstimate (application/signalstrength.cpp:287-380; receiver.cpp:891-892, 959-960) on every
 * frame's unprocessed spectrum, per channel: float4 (peakDb, avgDb, snrDb, floorDb) at [channel * pitch + frame].  The
 * band window is the channel's band-pass (+-100 kHz in a WFM bank) around its mixer frequency.  avgDb is the value the
 * reference's squelch compares with m_squelchDb (receiver.cpp:893-897, 962-965); see pebblegpu_set_squelch.
 * Needs spectrum_bins != 0.  The reference's 10-per-second update timer is open by default: every frame is measured.  With
 * pebblegpu_set_spectrum_updates: one float4 per COMPUTED row, indexed like the rows. */
int pebblegpu_receiver_enable_signal_strength(pebblegpu_receiver *rx, int on);
const void *pebblegpu_receiver_signal_strength(const pebblegpu_receiver *rx, uint64_t *frames, uint64_t *pitch_frames);
/* Squelch (Receiver::squelchChanged, receiver.cpp:704-707; the gate at :893-897 for WFM and :962-965 otherwise).  Once a
 * super-frame has been mixed, decimated and (narrow chains) band-passed, avgDb of the unprocessed spectrum of its last raw frame
 * is compared with squelch_db: below it the channel's processing ends there -- noise filter, AGC, demodulator and resampler
 * are not run and keep their state -- exactly the reference's early return.  -120 (DB::minDb, the reference's default) never
 * closes the gate.  Turns the S-meter on; needs spectrum_bins != 0.
 *   - the reference's own shape, one channel called one super-frame at a time (narrow or WFM): the call reports ZERO audio
 *     samples (pebblegpu_receiver_audio's n, process_iq's n_audio); the decision costs one 16-byte read-back and a stream
 *     synchronisation per call, made only while a threshold above -120 is set;
 *   - a narrow bank, or calls of several super-frames: one threshold per channel, the decision per (channel, super-frame) made on
 *     the device from the same call's spectra (no read-back, no synchronisation); a closed (channel, super-frame) reads as
 *     silence in the bank's audio rows (the count is common to all channels), and with audio_rate set the resampler sees that
 *     silence (a single Receiver's resampler would have slept).  A WFM receiver with more than one channel, or one created
 *     for several super-frames per call: a threshold above -120 is PEBBLEGPU_E_UNSUPPORTED (-120 and below, "never closes", is
 *     accepted and does nothing). */
int pebblegpu_set_squelch(pebblegpu_receiver *rx, uint32_t channel, double squelch_db);
/* ------------------------------------------------------------------------------------------------
 * Test bench on the batched device path: the generator at the head of Receiver::processIQData (application/receiver.cpp:797-798,
 * TestBench::genSweep then TestBench::genNoise, application/testbench.cpp:518-544 -> NCO::genSweep / NCO::genNoise,
 * pebblelib/nco.cpp:87-212) and taps at the points where the reference hands the signal to its scope (displayData, receiver.cpp:803,
 * 945, 953, 992) and to the digital modem (:979-980).  Everything is off by default; with both generators off and no tap set a call is
 * what it was before these entry points existed.  Batched path only: pebblegpu_process_iq, whose `in` is a host CPX * the host can
 * inject into and display itself, refuses a call while a generator or a tap is on (PEBBLEGPU_E_UNSUPPORTED).
 * ---------------------------------------------------------------------------------------------- */
typedef struct pebblegpu_sweep {            /* NCO::initSweep (nco.cpp:119-137) + what TestBench::genSweep passes (testbench.cpp:518-526) */
    uint32_t struct_size;                   /* = sizeof(pebblegpu_sweep) */
    int32_t  sweep_type;                    /* NCO::SweepType, nco.h:52: 0 SINGLE, 1 REPEAT, 2 REPEAT_REVERSE */
    double   start_hz, stop_hz, rate_hz_per_s;
    double   pulse_width_s, pulse_period_s; /* width <= 0: no pulse modulation (nco.cpp:149) */
    double   amplitude;                     /* m_signalAmplitude, linear (m_ampMax * dBToAmplitude(dB), testbench.cpp:563) */
    int32_t  mix;                           /* genMixBox (testbench.cpp:521): 1 add to the input, 0 replace it */
    uint32_t reserved[3];
} pebblegpu_sweep;
/* What the library makes of a sweep, on the host, no device needed: leg_samples = samples from the start frequency until the frequency
 * reaches the stop frequency (nco.cpp:188-189; 0: never -- rate <= 0 keeps the frequency, nco.cpp:181); pulse_period_samples /
 * pulse_on_samples = the reference's serial pulse timer (m_sweepPulseTimer += 1 / fs, reset once it exceeds the period, amplitude 0
 * while it exceeds the width, nco.cpp:149-156) run once in double as the reference runs it: of every pulse_period_samples samples the
 * first pulse_on_samples and the last one carry the signal (0, 0: no pulse modulation).  Refused: legs shorter than 64 samples and
 * pulse periods of 2^28 samples or more (PEBBLEGPU_E_UNSUPPORTED; the setter runs the timer's sum once, one addition per sample of a period), non-finite values, an unknown type (PEBBLEGPU_E_INVALID). */
int pebblegpu_sweep_plan(double sample_rate, const pebblegpu_sweep *s, uint64_t *leg_samples, uint64_t *pulse_period_samples,
                         uint64_t *pulse_on_samples);
/* TestBench::reset() + the generator switch of a receiver (s == NULL: sweep off).  Every call of either setter restarts the sweep at
 * start_hz with phase 0 and pulse timer 0 and the noise counter at 0.  From then on sample i of every stream gets
 * amp_i * (cos phi_i, sin phi_i): phi advances by f * 2 pi / fs per sample and f by rate / fs, with the three SweepType behaviours where f
 * reaches the stop frequency (nco.cpp:188-207).  The phase is evaluated in double from a closed form per sweep leg (DESIGN.md section
 * 4) instead of the reference's serial sum: they differ by the serial sum's own rounding (1e-7 rad over 2^18 samples at the rates
 * tested).  The sample is formed in double -- input + sweep + noise -- and rounded to float once.  The sweep is the same on every stream
 * of a receiver with independent streams.
 * A call with a generator on is staged: the caller's buffer is never written; raw formats are converted into the library's staging
 * buffer and generated into there, float2 input is read, summed and written into that buffer by the generator's own kernel.  Such a
 * call is never raw-fused and never pipelined with the calls around it (the staging buffer is shared by successive calls, as with
 * pebblegpu_set_conditioners); its chain may still run beside its own display transform, with the kernels of the same call without a
 * generator: its audio is bit for bit that of a receiver fed the summed stream.  pebblegpu_receiver_kernel_name(rx, 2) starts with
 * "k_testbench + ". */
int pebblegpu_set_testbench_sweep(pebblegpu_receiver *rx, const pebblegpu_sweep *s);
/* TestBench::genNoise -> NCO::genNoise (nco.cpp:87-116), always mixed (testbench.cpp:542); amplitude = m_noiseAmplitude, linear; <= 0:
 * off.  The reference draws from rand(); the library keeps the method (Knop's polar form, u = 1 - 2 r / 2147483647 with 31-bit r, s >= 1
 * or s == 0 rejected, sqrt(-2 ln s / s), in double) and makes r a pure function of (seed, stream, sample number since the last setter,
 * attempt, which of the two): splitmix64's finaliser, see DESIGN.md section 4 and tests/testbench_ref.py.  At most 32 attempts per
 * sample; a sample whose 32 attempts all fail (4e-22) gets no noise.  Streams of one receiver get different noise. */
int pebblegpu_set_testbench_noise(pebblegpu_receiver *rx, double amplitude, uint64_t seed);
/* Keyed Morse stations: the reference's plugins/MorseGenDevice, a bank of MorseGen objects (morsegen.cpp:33-328) summed at the head of
 * the chain (morsegendevice.cpp:1008-1063), here in the test bench's generator pass.  A station sends its tokens over and over: a token
 * is MorseCode's (a leading 1, then 1 per dash and 0 per dot, below 0x200: genToken shifts nine bits, morsegen.cpp:244), 0 is a word
 * space (' ', genText :226).  The application keeps MorseCode::asciiLookup, as it keeps tokenLookup on the decoder's side.
 * With msTcw = 1200 / wpm (integer, MorseCode::wpmToTcwMs), samplesPerTcw = (quint32)(msTcw / (1000.0 / fs)) and rise = fall =
 * (quint32)(ms_rise / (1000 / fs)) (morsegen.cpp:45-58), a dot is rise + (samplesPerTcw - rise) + fall samples and a dash
 * rise + (3 samplesPerTcw - rise) + fall (:59-67).  Inside a mark the carrier starts at phase 0 at the mark's first sample and advances
 * by 2 pi f / fs per sample (:90-142: it restarts at every dot and dash); the envelope rises as ampInc (i + 1) over the rise samples
 * (ampInc = amplitude / rise), holds at amplitude, and falls as amplitude - ampInc (i + 1), so that the last fall sample is 0.
 * samplesPerTcw zeros come between two marks of one character only (genDot / genDash :272-275), 3 samplesPerTcw zeros behind every
 * token (genChar), 7 samplesPerTcw - 3 zeros for a word space (the reference's "- 3" is in samples, :84) in addition to the character
 * space before it; the text starts over from its first token with nothing in between (nextOutputSample :204-207).
 * The library evaluates phase and ramps in closed form (phase in turns, reduced exactly; a lane makes a short run of samples from one
 * sincos and rotations in double): they differ from the reference's serial sums by those sums' own rounding.  DESIGN.md section 4.
 * Not built: the per-sample random fade (morsegendevice.cpp:1016-1021, libc's unseeded rand()), presets and the UI. */
#define PEBBLEGPU_MORSE_MAX_STATIONS 256    /* stations a receiver or a generator takes at most */
typedef struct pebblegpu_morse_station {    /* MorseGen::setParams + setTextOut (morsegen.cpp:33, 163) */
    uint32_t struct_size;                   /* = sizeof(pebblegpu_morse_station) */
    uint32_t wpm;
    uint32_t ms_rise;                       /* m_msRiseFall; 0: hard keying */
    uint32_t n_tokens;
    double   frequency_hz, amplitude;       /* amplitude linear: DB::dBToAmplitude(dbAmplitude), morsegen.cpp:40 */
    const uint16_t *tokens;                 /* n_tokens of them; copied by the setter */
    uint32_t reserved[2];
} pebblegpu_morse_station;
/* What the library makes of a station, on the host, no device needed: the lengths above in samples (dot_samples / dash_samples: the
 * whole mark buffers, rise and fall included) and period_samples, one pass through the text.  PEBBLEGPU_E_INVALID: a null or mis-sized
 * struct, non-finite values, |frequency| >= fs / 2, n_tokens == 0, a token of 0x200 or more.  PEBBLEGPU_E_UNSUPPORTED: wpm 0, msTcw or
 * samplesPerTcw 0, samplesPerTcw <= rise (a dot of less than one sample at full level: the reference's unsigned subtraction wraps), a
 * mark of 2^26 samples or more, a period of 2^40 samples or more.  Any of the output pointers may be NULL. */
int pebblegpu_morse_station_plan(double sample_rate, const pebblegpu_morse_station *st, uint64_t *samples_per_tcw, uint64_t *rise_samples,
                                 uint64_t *dot_samples, uint64_t *dash_samples, uint64_t *period_samples);
/* For parity checks, on the host, no device needed: the mark table the library builds for a call of n samples that begins first_sample
 * samples after the station was set -- for every mark that intersects the call, (start relative to the call's first sample) * 2 +
 * (1: dash), ascending; a mark that began before the call has a negative start.  *n_marks: how many there are (PEBBLEGPU_E_SIZE when
 * more than cap; more than 2^22 in one call: PEBBLEGPU_E_UNSUPPORTED, as the generating call itself). */
int pebblegpu_morse_station_marks(double sample_rate, const pebblegpu_morse_station *st, uint64_t first_sample, uint64_t n, int64_t *marks,
                                  uint32_t cap, uint32_t *n_marks);
/* Replaces the receiver's whole set of stations (n_stations == 0: off; more than PEBBLEGPU_MORSE_MAX_STATIONS: PEBBLEGPU_E_INVALID) and
 * starts every station at its first token with the next sample.  It does not restart the sweep or the noise counter, and the two setters
 * above do not restart the stations.  mix = 1 adds the stations to the input; mix = 0: the caller's input is not read.  With the sweep
 * on as well the input is dropped when either says "replace"; sweep, stations and noise are summed in double and rounded to float once.
 * The stations are the same on every stream of a receiver with independent streams (their sum is formed once per sample position).  A
 * call with stations on is staged exactly as a call with the sweep on (see pebblegpu_set_testbench_sweep);
 * pebblegpu_receiver_kernel_name(rx, 2) then starts with "k_morsegen + " (the kernel that also makes the call's sweep and noise).  A
 * refused call leaves the set as it was. */
int pebblegpu_set_testbench_morse(pebblegpu_receiver *rx, const pebblegpu_morse_station *stations, uint32_t n_stations, int mix);
/* Taps: the float2 signal of the whole call at a point of the chain, copied into a library-owned buffer (allocated when the point is
 * first enabled) by a copy queued on the call's stream at that point.  Valid after pebblegpu_receiver_synchronize until the next call.
 *   RAW_IQ      [stream][n_samples] at the stream rate: the streams after the generator, before the conditioners (receiver.cpp:803)
 *   POST_MIXER  [channel][n_samples / D] at the demodulator rate: the decimated frames after the gain restore, what zoomed() sees
 *               (receiver.cpp:942-945; on a WFM receiver m_sampleBuf at :884)
 *   POST_BP     [channel][n_samples / D]: the band-pass output (receiver.cpp:953)
 *   MODEM       [channel][n_samples / D]: after NoiseFilter::ProcessBlock, the frame m_iDigitalModem->processBlock receives (:974-980)
 *   POST_DEMOD  [channel][n_samples / D]: the demodulator output before the resampler (receiver.cpp:992)
 * Channels in dmNONE leave their MODEM and POST_DEMOD rows zero (the reference returns before, :968-971).  A tap changes no value and
 * no kernel of the call; a receiver without a display transform runs a call with taps on one stream instead of as two overlapping
 * stages.  Refused (PEBBLEGPU_E_UNSUPPORTED, nothing changed): POST_BP, MODEM and POST_DEMOD on a WFM receiver (it has no such
 * points); MODEM or POST_DEMOD together with a squelch threshold above -120, by whichever setter comes second (a closed gate ends the
 * call before those points).  mask: 1 << point or'ed; 0 switches every tap off. */
enum { PEBBLEGPU_TAP_RAW_IQ = 1, PEBBLEGPU_TAP_POST_MIXER = 2, PEBBLEGPU_TAP_POST_BP = 3, PEBBLEGPU_TAP_POST_DEMOD = 4,   /* TB_RAW_IQ .., receiver.h:113-116 */
       PEBBLEGPU_TAP_MODEM = 16 };                                                                                        /* receiver.cpp:979-980 */
int pebblegpu_receiver_set_taps(pebblegpu_receiver *rx, uint32_t mask);
/* the tap's row 0 after the last call (NULL: the point is off, or the last call did not reach it); row r starts *pitch_samples float2 further */
const void *pebblegpu_receiver_tap(const pebblegpu_receiver *rx, int point, uint64_t *samples_per_row, uint64_t *pitch_samples, double *rate);
/* waits until every process call made on this handle has finished: its outputs are then valid and its input may be reused */
int pebblegpu_receiver_synchronize(pebblegpu_receiver *rx);

/* Host single-frame path with the reference's callback shape:
 *   CB_ProcessIQData  = std::function<void(CPX*, quint16)>  (pebblelib/device_interfaces.h:32)
 *   CB_ProcessAudioData same shape (device_interfaces.h:38).
 * One frame of n == frames_per_buffer samples for channel/stream 0 in; frames accumulate until a whole
 * super-frame is present (the reference returns early until m_sampleBuf is full, receiver.cpp:922-931);
 * then *n_audio = frames_per_buffer (more for FastFIR variants) and audio holds left/right doubles.  Otherwise *n_audio = 0.
 * spectrum_db (may be NULL) receives this frame's dB spectrum (bins doubles). */
int pebblegpu_process_iq(pebblegpu_receiver *rx, const double *iq, uint16_t n, double *audio,
                         uint32_t *n_audio, double *spectrum_db);
/* The same for a host that has called pebblegpu_set_spectrum_updates: *spectrum_updated (may be NULL) is 1 when this frame got a
 * spectrum -- spectrum_db was written -- and 0 when the update timer skipped it: spectrum_db is then left untouched, so a host that
 * passes the same buffer every frame keeps the last computed spectrum in it, as SignalSpectrum::getUnprocessed does.  Without a gate
 * every frame reports 1 (when spectrum_db was asked for).  pebblegpu_process_iq itself leaves spectrum_db untouched in the same way. */
int pebblegpu_process_iq_updates(pebblegpu_receiver *rx, const double *iq, uint16_t n, double *audio,
                                 uint32_t *n_audio, double *spectrum_db, uint32_t *spectrum_updated);

/* ------------------------------------------------------------------------------------------------
 * Multibank: ONE process and ONE consumer thread drive a bank whose channels are sharded across several devices (what a host
 * behind the reference's plugin surface is: Receiver::turnPowerOn builds one chain, application/receiver.cpp:116-281, and
 * processIQData is called from one thread).  Shard g of G owns the global channels [g*C/G, (g+1)*C/G) in integer arithmetic
 * (4096 over 8: 512 each; 5 over 2: [0,2) and [2,5)); pebblegpu_multibank_plan is that rule, on the host, no device needed.
 * Each shard is an ordinary pebblegpu_receiver created on device_ids[g] with the caller's configuration and the shard's channel
 * count (cfg->n_channels is the total C, cfg->device is ignored; with shared_input = 0 the streams are split by the same ranges), so
 * every sample goes through exactly the kernels a single-device bank runs, and nothing is exchanged between devices.
 *   - A device may appear more than once in device_ids: {0, 0} is two shards on one device.  That is a TEST RIG for machines with
 *     one GPU -- two shards on one device share it and run slower than one bank of the same channels -- not a configuration to run.
 *   - PEBBLEGPU_MULTIBANK_SPECTRUM_SHARD0: shards 1.. are created with spectrum_bins = hires_bins = 0 (with a shared stream every
 *     shard's display transform would compute the same rows).  What reads the spectrum (S-meter, squelch) then works on shard 0 and
 *     is refused on the others exactly as on a single bank without one.  Without the flag every shard has its spectrum.
 *   - Setters and read-outs are not duplicated: pebblegpu_multibank_shard hands out the shard's receiver handle, BORROWED, and every
 *     pebblegpu_set_* and pebblegpu_receiver_* read-out works on (rx, channel - first_channel); pebblegpu_multibank_locate does the
 *     arithmetic.  As on a single receiver, setters may be called from another thread and take effect at the next call.  A borrowed
 *     handle must NOT be passed to pebblegpu_receiver_destroy, nor to any process / ingest entry point (pebblegpu_receiver_process,
 *     _process_raw, _ingest_acquire, _ingest_submit, _process_ingested, pebblegpu_process_iq, _process_iq_updates): those belong to
 *     the multibank; it is valid until pebblegpu_multibank_destroy.  Outputs stay sharded: each shard's audio is on its device.
 *     The audio blocks and recorded IQ (pebblegpu_receiver_audio_out_*, pebblegpu_set_audio_level, pebblegpu_receiver_record_*, below)
 *     are such setters and read-outs: they work per shard on the borrowed handle, and there is no multibank call for them.
 *   - create checks its arguments before any device is touched (PEBBLEGPU_E_INVALID: a null pointer, a struct_size mismatch,
 *     n_shards 0 or above PEBBLEGPU_MULTIBANK_MAX_SHARDS, n_channels < n_shards, unknown flag bits), then probes the devices
 *     (PEBBLEGPU_E_NO_DEVICE with none, PEBBLEGPU_E_INVALID for an ordinal out of range).
 *   - Every shard has a persistent host worker thread (created by create, joined by destroy -- hence the cap of 16: a node has 8
 *     devices).  A process call posts its job to all workers and returns when ALL HAVE QUEUED their shard's call, not when the
 *     calls have run: the ASYNCHRONY rules above hold unchanged, with pebblegpu_multibank_synchronize in the place of
 *     pebblegpu_receiver_synchronize.  Process calls are single-caller per multibank handle.
 *   - The common checks are made once, before any worker is asked -- null pointers, the state of an ingest slot, n_samples a whole
 *     number of super-frames (PEBBLEGPU_E_SIZE) and at most max_superframes -- and a refusal there leaves every shard untouched and
 *     the handle usable.  A failing shard's error text is carried to the calling thread's pebblegpu_last_error() and the call
 *     returns the first failing shard's code.  If a shard refuses or fails AFTER others have queued, the shards' streams no longer
 *     agree: the multibank is failed, later process calls return PEBBLEGPU_E_HIP with a text that says so, and only
 *     pebblegpu_multibank_synchronize and _destroy (and the read-outs of the shards) still work.
 *   - destroy waits for every shard's queued work, stops the workers, then destroys the shards; it may be called right behind a
 *     queued call.
 * ---------------------------------------------------------------------------------------------- */
typedef struct pebblegpu_multibank pebblegpu_multibank;
#define PEBBLEGPU_MULTIBANK_MAX_SHARDS 16
#define PEBBLEGPU_MULTIBANK_SPECTRUM_SHARD0 1u   /* flags bit 0 */
/* first[g], count[g] for g < n_shards: contiguous, covering [0, n_channels), none empty.  PEBBLEGPU_E_INVALID: a null pointer,
 * n_shards 0 or above 16, n_channels < n_shards. */
int pebblegpu_multibank_plan(uint32_t n_channels, uint32_t n_shards, uint32_t *first, uint32_t *count);
int pebblegpu_multibank_create(const pebblegpu_config *cfg, const int32_t *device_ids, uint32_t n_shards,
                               uint32_t flags, pebblegpu_multibank **out);
int pebblegpu_multibank_destroy(pebblegpu_multibank *mb);
int pebblegpu_multibank_shards(const pebblegpu_multibank *mb, uint32_t *n_shards);
/* shard g: a BORROWED receiver handle (see above), its device, its first global channel and its channel count; any of the four
 * output pointers may be NULL */
int pebblegpu_multibank_shard(pebblegpu_multibank *mb, uint32_t g, pebblegpu_receiver **rx, int32_t *device,
                              uint32_t *first_channel, uint32_t *n_channels);
/* global channel -> (shard, channel within the shard); PEBBLEGPU_E_INVALID for a channel out of range */
int pebblegpu_multibank_locate(const pebblegpu_multibank *mb, uint32_t channel, uint32_t *shard, uint32_t *local_channel);
/* Device-resident input: d_iq / d_raw is an array of n_shards device pointers; entry g is resident on shard g's device and holds what
 * that shard reads, as pebblegpu_receiver_process / _process_raw take it -- the whole stream for a shared stream (with {0, 0} both
 * entries may be the same pointer), the shard's rows [stream][time] for independent streams.  A host that keeps its samples on one
 * device distributes them itself.  The inputs are never modified and may be overwritten after pebblegpu_multibank_synchronize.
 * Every d_raw entry must be aligned to PEBBLEGPU_RAW_ALIGN bytes, as for pebblegpu_receiver_process_raw; a misaligned one is refused
 * (PEBBLEGPU_E_INVALID) before any shard is asked, so the multibank stays usable. */
int pebblegpu_multibank_process(pebblegpu_multibank *mb, const void *const *d_iq, uint64_t n_samples);
int pebblegpu_multibank_process_raw(pebblegpu_multibank *mb, int format, int iq_order, double gain,
                                    const void *const *d_raw, uint64_t n_samples);
/* Host ingest, the path a one-process host really has (samples arrive from a radio in host memory): two pinned slots owned by the
 * multibank, readable by every device, with the contract of pebblegpu_receiver_ingest_* above.
 *   acquire  -- blocks until every shard's last call that read the slot's device twin is over, then hands out the slot's buffer;
 *   submit   -- queues one upload per shard, on that shard's copy stream, into that shard's device twin: all `bytes` for a shared
 *               stream; for independent streams the buffer is [stream][time] in n_channels equal rows and each shard is sent its
 *               rows only (bytes must then be n_channels * n_samples pairs exactly);
 *   process_ingested -- pebblegpu_receiver_process_raw per shard on its twin, ordered behind that shard's upload on the device, no
 *               host synchronisation.  Refused, with every shard untouched: a slot nothing was submitted to or too small for the
 *               format (PEBBLEGPU_E_SIZE), a slot whose samples have been processed and that has not been acquired since
 *               (PEBBLEGPU_E_INVALID).
 * Copies from host memory per shard, not peer copies from an ingest device: the same code runs on one device and on eight, it
 * depends on no peer-access state, and the traffic is small. */
int pebblegpu_multibank_ingest_acquire(pebblegpu_multibank *mb, uint32_t slot, uint64_t bytes, void **host_ptr);
int pebblegpu_multibank_ingest_submit(pebblegpu_multibank *mb, uint32_t slot, uint64_t bytes);
int pebblegpu_multibank_process_ingested(pebblegpu_multibank *mb, uint32_t slot, int format, int iq_order,
                                         double gain, uint64_t n_samples);
/* waits until every call made on this handle has finished on every shard */
int pebblegpu_multibank_synchronize(pebblegpu_multibank *mb);
/* the maximum over the shards of pebblegpu_receiver_last_ms(rx, 0, ..): the slowest shard bounds the call */
int pebblegpu_multibank_last_ms(const pebblegpu_multibank *mb, float *max_over_shards);

/* ------------------------------------------------------------------------------------------------
 * Stream bank: S independent full-rate IQ streams, each through the overlap-save band-pass
 * (CFastFIR::ProcessData, pebblelib/fastfir.cpp:281-334, one filter per stream) and the display
 * transform (FFT::fftSpectrum, pebblelib/fft.cpp:317-374) at the stream rate -- the two transforms of
 * Receiver::processIQData with no tuner/decimator in front (BASELINE.json configs[4]: 1024 streams over 8 GPUs,
 * 128 per GPU, 65536-point spectrum, 2048/1025 band-pass).  Device buffers, one process per GPU, streams shard
 * across ranks with no exchange.  frame/spectrum_bins: 2048-sample frames with 2048/4096/8192 bins
 * (the reference's setup), or 65536/65536, which is past the reference's own m_maxFFTSize clamp
 * (fft.h:21) and uses the same formulas with the clamp lifted.
 * ---------------------------------------------------------------------------------------------- */
typedef struct pebblegpu_streambank pebblegpu_streambank;
typedef struct pebblegpu_streambank_config {
    uint32_t struct_size;
    int32_t device;
    double sample_rate;      /* stream rate, used by the band-pass design (fastfir.cpp:186-261) */
    uint32_t n_streams;
    uint32_t frame;          /* samples per spectrum frame */
    uint32_t spectrum_bins;
    uint32_t fastfir_fft;    /* 0 -> 2048; 2048, 4096 or 8192 */
    uint32_t fastfir_taps;   /* 0 -> 1025; 2 .. fastfir_fft/2 + 1, else PEBBLEGPU_E_INVALID (overlap taps-1 <= block fft-overlap);
                                frame must be a multiple of the block */
    uint32_t max_frames;     /* capacity per call, frames per stream */
    uint32_t reserved[5];
} pebblegpu_streambank_config;
int pebblegpu_streambank_create(const pebblegpu_streambank_config *cfg, pebblegpu_streambank **out);
int pebblegpu_streambank_destroy(pebblegpu_streambank *sb);
/* CFastFIR::SetupParameters(lo, hi, 0, sample_rate) for one stream; E_FILTER_PARAM on the reference's
 * "Filter Parameter error" (fastfir.cpp:201-208), the previous filter stays in place */
int pebblegpu_streambank_set_bandpass(pebblegpu_streambank *sb, uint32_t stream, double lo, double hi);
/* d_iq: [stream][n_samples] float2, n_samples a multiple of frame.  what: bit 0 band-pass, bit 1 spectrum */
int pebblegpu_streambank_process(pebblegpu_streambank *sb, const void *d_iq, uint64_t n_samples, uint32_t what);
/* filtered [stream][n_samples] float2 (row pitch returned); spectrum [stream][frames][bins] float dB (under an update gate, below:
 * the computed frames only) */
const void *pebblegpu_streambank_filtered(const pebblegpu_streambank *sb, uint64_t *samples_per_stream, uint64_t *pitch_samples);
const void *pebblegpu_streambank_spectrum(const pebblegpu_streambank *sb, uint64_t *frames_per_stream, uint32_t *bins);
/* which: 0 whole call, 1 band-pass kernel, 2 spectrum kernels */
int pebblegpu_streambank_last_ms(const pebblegpu_streambank *sb, int which, float *ms);
int pebblegpu_streambank_synchronize(pebblegpu_streambank *sb);
/* pebblegpu_streambank_process on streams still in the device's sample format: d_raw is [stream][n_samples] IQ pairs of `format`
 * (pebblegpu_iq_format; row pitch n_samples pairs), converted as DeviceInterfaceBase::normalizeIQ does (format / iq_order / gain as in
 * pebblegpu_receiver_process_raw; gain 0 is silence).  Results equal pebblegpu_streambank_process on the same samples converted on the
 * host, bit for bit, and raw and float2 calls may alternate on one bank: the band-pass's overlap carries converted samples.
 * With 65536-sample frames and 65536 bins, or 2048-sample frames and 8192 bins, and the 2048-point band-pass, both kernels convert in
 * their own loads and no float2 copy of the streams exists; every other geometry is converted by one pass into a library-owned
 * float2 buffer first (allocated on the first such call).  Only the kernels the call asks for count (`what`): a band-pass-only call
 * on the 2048-point band-pass converts in its loads whatever the display geometry.  pebblegpu_streambank_kernel_name tells which.
 * d_raw must be aligned to PEBBLEGPU_RAW_ALIGN bytes (the kernels read it with loads of up to 32 bytes).  Refused before anything is
 * queued, leaving the handle usable: unknown format or order (PEBBLEGPU_E_INVALID), n_samples not a multiple of the frame or above the
 * capacity (PEBBLEGPU_E_SIZE), a misaligned d_raw (PEBBLEGPU_E_INVALID). */
#define PEBBLEGPU_RAW_ALIGN 32
int pebblegpu_streambank_process_raw(pebblegpu_streambank *sb, int format, int iq_order, double gain, const void *d_raw, uint64_t n_samples,
                                     uint32_t what);
/* The library's pinned double buffer for a stream bank, same contract as pebblegpu_receiver_ingest_* above:
 * acquire(slot, bytes) hands out the slot's pinned host buffer (after waiting for the call that last read the slot), the host writes
 * [stream][n_samples] raw pairs into it, submit(slot, bytes) queues the upload, process_ingested runs pebblegpu_streambank_process_raw
 * on the uploaded samples behind the upload -- while the host fills the other slot.  Refused: a slot submitted again without an
 * acquire while its call is in flight (PEBBLEGPU_E_INVALID), more bytes than acquired, or a format whose n_streams * n_samples pairs
 * do not fit the submitted bytes (PEBBLEGPU_E_SIZE). */
int pebblegpu_streambank_ingest_acquire(pebblegpu_streambank *sb, uint32_t slot, uint64_t bytes, void **host_ptr);
int pebblegpu_streambank_ingest_submit(pebblegpu_streambank *sb, uint32_t slot, uint64_t bytes);
int pebblegpu_streambank_process_ingested(pebblegpu_streambank *sb, uint32_t slot, int format, int iq_order, double gain, uint64_t n_samples,
                                          uint32_t what);
/* which: 1 band-pass, 2 display transform -> the kernel route the LAST call took ("" when the call did not ask for it), stable names
 * as pebblegpu_receiver_kernel_name: e.g. "k_fastfir_t128 (raw s8)" for converting loads against "k_normalize_iq + k_fastfir_t128"
 * for a staged raw call and "k_fastfir_t128" for float2 input */
const char *pebblegpu_streambank_kernel_name(const pebblegpu_streambank *sb, int which);
/* FFT::mapFFTToScreen (see pebblegpu_screen_map above) of frames first_frame + j * frame_step (j < n_frames) of every stream of the
 * last call's spectrum (sampleRate = the bank's sample_rate, fftSize = spectrum_bins; 65536 with the clamp lifted) into the device
 * buffer d_out: int32 [stream][n_frames][x_pixels].  Queued behind the call's transform on the bank's stream; d_out holds the result
 * after pebblegpu_streambank_synchronize. */
int pebblegpu_streambank_map_spectrum(pebblegpu_streambank *sb, const pebblegpu_screen_map *map, uint32_t first_frame, uint32_t n_frames,
                                      uint32_t frame_step, int32_t *d_out);
/* The spectrum's update gate for a stream bank: pebblegpu_set_spectrum_updates (above; its comment is the specification) with ONE
 * timer per bank on the bank's sample clock -- all streams share it, so all select the same frames; the rate of the rule is
 * sample_rate rounded to the nearest whole Hz, frames_per_buffer is `frame`.  PEBBLEGPU_SPECTRUM_EVERY_FRAME (-1, the default): every
 * frame, exactly as without this setter; 0: no spectrum; a negative rate other than -1 is PEBBLEGPU_E_INVALID.  Changing the rate
 * changes the period only, the timer runs on.  With a gate set:
 *   - the frame list is worked out on the host before anything is queued (no read-back, no synchronisation), for every process call:
 *     pebblegpu_streambank_process, _process_raw and _process_ingested (raw and float2 results stay equal bit for bit);
 *   - pebblegpu_streambank_spectrum returns the COMPUTED rows only, compact: [stream][n_selected][bins]; the frame count it reports is
 *     n_selected and may be 0; a row is averaged with the previous COMPUTED row's amplitudes (fft.cpp:378-386), across calls; a call
 *     that selects nothing launches no transform and leaves those amplitudes alone;
 *   - pebblegpu_streambank_map_spectrum indexes the compact rows; after a call that asked for the spectrum (bit 1) and selected nothing it
 *     maps the latest row computed before it, as frame 0 with n_frames = 1 (refused before any row has been computed); after a call
 *     without bit 1 it is refused, gate or no gate;
 *   - pebblegpu_streambank_last_ms(sb, 2) is valid (nothing elapsed when nothing ran), pebblegpu_streambank_kernel_name(sb, 2) names the
 *     frame-list kernels ("k_big256_cols_list + k_big256_rows", "k_spectrum_list_q128", "k_spectrum_list_any", with " (raw ...)" or
 *     "k_normalize_iq + " as for the every-frame kernels) and is "" after a call that selected nothing;
 *   - the band-pass output is the same on every route, bit for bit.
 * A call WITHOUT bit 1 of `what` advances the sample clock by its frames and nothing else: it selects no frame and neither starts nor
 * restarts the timer (under the default as well: a later gate counts from the last frame that did get a spectrum). */
int pebblegpu_streambank_set_spectrum_updates(pebblegpu_streambank *sb, int updates_per_sec);
/* which frames of the last call got a spectrum: indices relative to the call's first frame, ascending, row i of the spectrum buffer
 * belongs to idx[i].  Without a gate every frame of the last call (none when it did not ask for the spectrum); *n = 0 before any call;
 * PEBBLEGPU_E_SIZE when cap is too small.  Known the moment the process call returns. */
int pebblegpu_streambank_spectrum_frames(const pebblegpu_streambank *sb, uint32_t *idx, uint32_t cap, uint32_t *n);

/* ------------------------------------------------------------------------------------------------
 * Stand-alone process steps with the reference's per-class call shapes, host buffers in and out.
 * These back the C++ adapter classes in include/pebblegpu_steps.hpp.
 * ---------------------------------------------------------------------------------------------- */
typedef struct pebblegpu_mixer pebblegpu_mixer;
/* Mixer::Mixer(sampleRate, bufferSize), mixer.cpp:5-17 */
int pebblegpu_mixer_create(int device, uint32_t sample_rate, uint32_t buffer_size, pebblegpu_mixer **out);
int pebblegpu_mixer_destroy(pebblegpu_mixer *m);
int pebblegpu_mixer_set_frequency(pebblegpu_mixer *m, double f);                 /* mixer.cpp:25-40 */
/* CPX *Mixer::processBlock(CPX *in), pebblelib/mixer.h:15: *out = library buffer, or = in when f == 0 */
int pebblegpu_mixer_process(pebblegpu_mixer *m, const double *in, const double **out);

typedef struct pebblegpu_decimator pebblegpu_decimator;
/* Decimator::Decimator + buildDecimationChain, decimator.cpp:6-46, 64-149 */
int pebblegpu_decimator_create(int device, uint32_t sample_rate, uint32_t buffer_size, pebblegpu_decimator **out);
int pebblegpu_decimator_destroy(pebblegpu_decimator *d);
int pebblegpu_decimator_build_chain(pebblegpu_decimator *d, uint32_t sample_rate_in, uint32_t protect_bw,
                                    uint32_t sample_rate_out, float *achieved_rate);
int pebblegpu_decimator_dec_by2_stages(const pebblegpu_decimator *d, uint32_t *stages);
/* quint32 Decimator::process(CPX *in, CPX *out, quint32 n), pebblelib/decimator.h:238.  n must be a multiple of
 * the total decimation.  Streams with exact history for any such n: a frame shorter than a stage's tap count is NOT
 * degraded to sample dropping (the reference's fallback, decimator.cpp:602-625, reads indeterminate memory) --
 * see DESIGN.md section 4. */
int pebblegpu_decimator_process(pebblegpu_decimator *d, const double *in, double *out, uint32_t n, uint32_t *n_out);

typedef struct pebblegpu_downconvert pebblegpu_downconvert;
/* CDownConvert (pebblelib/downconvert.h:25-50, downconvert.cpp): the alternate mixer + decimator -- a quadrature oscillator
 * (the same recurrence as Mixer, but SetFrequency keeps its phasor and there is no "frequency 0 returns the input" exit) and a
 * cascade of decimate-by-2 stages picked per octave: CIC3, a fixed 11-tap halfband, 15..51-tap halfbands whose DecBy2 counts
 * tap 0 twice (downconvert.cpp:368-376: reproduced).  max_in_length: the largest InLength a ProcessData call will pass. */
int pebblegpu_downconvert_create(int device, uint32_t max_in_length, pebblegpu_downconvert **out);
int pebblegpu_downconvert_destroy(pebblegpu_downconvert *d);
/* TYPEREAL SetDataRate(InRate, MaxBW) (simple = 0, downconvert.cpp:139-206) / SetDataRateSimple (simple = 1, :213-237): builds
 * the stage list when either argument changed, returns the output rate.  As in the reference the call ends with
 * SetFrequency(m_NcoFreq) on the STORED frequency, which mirrors an earlier tuning (call it first, as receiver.cpp:198 does).
 * More than nine stages (the reference's pointer array holds ten entries including the terminating NULL): E_UNSUPPORTED. */
int pebblegpu_downconvert_set_data_rate(pebblegpu_downconvert *d, double in_rate, double max_bw, int simple, double *out_rate);
int pebblegpu_downconvert_set_frequency(pebblegpu_downconvert *d, double nco_freq);   /* SetFrequency, downconvert.cpp:100-112 */
int pebblegpu_downconvert_set_cw_offset(pebblegpu_downconvert *d, double offset);     /* SetCwOffset, downconvert.h:34 */
/* the stage list: taps[j] = tap count of stage j, 0 for the CIC3 */
int pebblegpu_downconvert_stages(const pebblegpu_downconvert *d, uint32_t *n_stages, uint32_t *taps, uint32_t taps_cap);
/* int ProcessData(int InLength, TYPECPX *pInData, TYPECPX *pOutData), downconvert.cpp:250-335: InLength a multiple of 2^stages;
 * returns the output count in *n_out.  The input is NOT modified (the reference mixes it in place).  Streams with exact history for
 * any such InLength: a call that leaves a stage fewer samples than it has taps is not skipped as the reference's "safety net" does
 * (:361-362, which returns stale samples).  Exact history is also NOT the reference wherever a stage of T taps is left T <= n < 2 (T - 1)
 * samples (n <= 18 for the fixed 11-tap stage): ProcessData runs its stages in place (:325) and DecBy2 copies its next history out of
 * pInData after its outputs have overwritten the front of it (:389-390).  Measured against the reference's own class over six equal
 * calls, from the second call on: 384 kHz / 8 kHz (11, 15, 23, 51 taps) in calls of 512: 7e-4 .. 3e-3 relative RMS, in calls of 1024
 * bit for bit; 256 kHz / 8 kHz (15, 19, 35) in calls of 256: 2e-6 .. 1e-5, in calls of 512 bit for bit (tests/test_oracle_pins.py,
 * tests/reference_cases.py DC_BOUNDARY). */
int pebblegpu_downconvert_process(pebblegpu_downconvert *d, uint32_t in_length, const double *in, double *out, uint32_t *n_out);
/* the same on device buffers (float2 in; *d_out: library-owned float2 row, valid until the next call); queues and returns */
int pebblegpu_downconvert_process_device(pebblegpu_downconvert *d, const void *d_iq, uint32_t in_length, const void **d_out, uint32_t *n_out);
int pebblegpu_downconvert_synchronize(pebblegpu_downconvert *d);

typedef struct pebblegpu_fastfir pebblegpu_fastfir;
/* CFastFIR::CFastFIR, fastfir.cpp:77-145 (fft/fir sizes are #defines there; 0,0 -> 2048,1025).  fft_size 2048, 4096 or 8192;
 * fir_size 2 .. fft_size/2 + 1, else PEBBLEGPU_E_INVALID: with a longer filter the overlap (fir_size-1) exceeds the block
 * (fft_size - overlap), where the reference's own bookkeeping no longer computes the convolution */
int pebblegpu_fastfir_create(int device, uint32_t fft_size, uint32_t fir_size, pebblegpu_fastfir **out);
int pebblegpu_fastfir_destroy(pebblegpu_fastfir *f);
/* void CFastFIR::SetupParameters(FLoCut, FHiCut, Offset, SampleRate), pebblelib/fastfir.h:57 */
int pebblegpu_fastfir_setup(pebblegpu_fastfir *f, double lo, double hi, double offset, double sample_rate);
/* int CFastFIR::ProcessData(int InLength, CPX *in, CPX *out), pebblelib/fastfir.h:59: *n_out samples written */
int pebblegpu_fastfir_process(pebblegpu_fastfir *f, int n, const double *in, double *out, int *n_out);

typedef struct pebblegpu_demod pebblegpu_demod;
/* Demod::Demod(sampleRate, wfmSampleRate, bufferSize), application/demod.cpp:49-69 */
int pebblegpu_demod_create(int device, uint32_t sample_rate, uint32_t wfm_sample_rate, uint32_t buffer_size,
                           pebblegpu_demod **out);
int pebblegpu_demod_destroy(pebblegpu_demod *d);
int pebblegpu_demod_set_mode(pebblegpu_demod *d, int mode);          /* demod.cpp:241-257 */
int pebblegpu_demod_set_bandwidth(pebblegpu_demod *d, double bw);    /* demod.cpp:230-239 */
/* CPX *Demod::processBlock(CPX *in, int n), application/demod.h:33: *out = library buffer, or = in for the
 * pass-through modes (demod.cpp:127-138).  The demodulating modes take calls of 80 samples or more (the depth of their FIRs' history);
 * a shorter one is PEBBLEGPU_E_SIZE and leaves the stream where it was.  dmFMS: a call is one block of processDataStereo and must be a
 * multiple of the RDS down-converter's decimation that leaves every stage at least its taps (PEBBLEGPU_E_SIZE otherwise, before anything
 * is queued).  Such calls stream with exact history; where they leave a stage fewer than 2 (T - 1) samples (calls of 512 and 768 at
 * 384 kHz, of 144 .. 264 at 256 kHz) the reference's in-place history differs -- by 7e-4 .. 3e-3 of the RDS branch's input at 384 kHz in
 * calls of 512, 2e-6 .. 1e-5 at 256 kHz in calls of 256 (see pebblegpu_downconvert_process) -- and a RECEIVER refuses the mode for
 * such a frame (pebblegpu_set_demod_mode) */
int pebblegpu_demod_process(pebblegpu_demod *d, const double *in, int n, const double **out);
/* dmFMS: getNextRdsGroupData as above, a processBlock call being one frame; and m_RdsData (the matched filter's output the bit
 * slicer reads, demod_wfm.cpp:309) of the last processBlock call: *n its length, at most cap values copied */
int pebblegpu_demod_rds_groups(pebblegpu_demod *d, pebblegpu_rds_group *groups, uint8_t *changed, uint32_t cap, uint32_t *n);
int pebblegpu_demod_rds_signal(pebblegpu_demod *d, double *data, uint32_t cap, uint32_t *n);
int pebblegpu_demod_stereo_lock(pebblegpu_demod *d, int *pilot_lock, int *changed);  /* getStereoLock, as above */

typedef struct pebblegpu_spectrum pebblegpu_spectrum;
/* FFT::factory + fftParams(fftSize, 0, sampleRate, samplesPerBuffer, BLACKMANHARRIS), fft.cpp:45-118 */
int pebblegpu_spectrum_create(int device, uint32_t fft_size, double sample_rate, uint32_t samples_per_buffer,
                              pebblegpu_spectrum **out);
int pebblegpu_spectrum_destroy(pebblegpu_spectrum *s);
int pebblegpu_spectrum_bins(const pebblegpu_spectrum *s, uint32_t *bins);
/* bool FFT::fftSpectrum(CPX *in, double *out, int numSamples), pebblelib/fft.h:38; *overload = return value */
int pebblegpu_spectrum_process(pebblegpu_spectrum *s, const double *in, int n, double *out_db, int *overload);
/* bool FFT::mapFFTToScreen(double *inBuf, ...), pebblelib/fft.h:53-56, with inBuf = the out of the last pebblegpu_spectrum_process
 * (what SignalSpectrum always passes): that spectrum, exactly the floats the call handed out as doubles, mapped on the device into
 * the host buffer out (x_pixels int32); sampleRate is the one the object was created with.  Blocks until out is written. */
int pebblegpu_spectrum_map_to_screen(pebblegpu_spectrum *s, const pebblegpu_screen_map *map, int32_t *out);

typedef struct pebblegpu_morse pebblegpu_morse;
/* Morse (DigitalModemInterface) + setSampleRate(sample_rate, sample_count), morse.cpp:160-246: the decoder as above on one stream */
int pebblegpu_morse_create(int device, uint32_t sample_rate, uint32_t sample_count, pebblegpu_morse **out);
int pebblegpu_morse_destroy(pebblegpu_morse *m);
int pebblegpu_morse_set_demod_mode(pebblegpu_morse *m, int mode);  /* Morse::setDemodMode, morse.cpp:337-341 */
/* CPX *Morse::processBlock(CPX *in), morse.cpp:761-894: one frame of sample_count CPX; the reference returns in unchanged */
int pebblegpu_morse_process(pebblegpu_morse *m, const double *in);
int pebblegpu_morse_events(pebblegpu_morse *m, pebblegpu_morse_event *ev, uint32_t cap, uint32_t *n);
int pebblegpu_morse_status(pebblegpu_morse *m, pebblegpu_morse_report *st);
/* Morse::setSampleRate again (every powerOn of the reference): a fresh decoder in dmCWL, with new frames if sample_count changed, that
 * starts from the current WPM estimate (the plugin object keeps m_wpmSpeedCurrent, morse.h:223).  Events decided before stay readable. */
int pebblegpu_morse_set_sample_rate(pebblegpu_morse *m, uint32_t sample_rate, uint32_t sample_count);
/* for parity checks: on != 0 makes every later process call also collect, per Goertzel result, m_power and the above-threshold decision
 * (off by default: nothing is kept); pebblegpu_morse_results hands them out since its last call (*n <= cap; the rest stays) */
int pebblegpu_morse_keep_results(pebblegpu_morse *m, int on);
int pebblegpu_morse_results(pebblegpu_morse *m, double *power, uint8_t *tone, uint32_t cap, uint32_t *n);

typedef struct pebblegpu_siggen pebblegpu_siggen;
/* The test bench's generator as a stand-alone step: NCO::NCO(sampleRate, bufSize) (nco.cpp:4-25) with initSweep / genSweep / genNoise,
 * the same kernel a receiver runs, on one stream of the caller's.  frames_per_buffer: the frame pebblegpu_siggen_generate expects most
 * often (its staging grows on demand). */
int pebblegpu_siggen_create(int device, double sample_rate, uint32_t frames_per_buffer, pebblegpu_siggen **out);
int pebblegpu_siggen_destroy(pebblegpu_siggen *g);
/* as pebblegpu_set_testbench_sweep / _noise: each call is TestBench::reset() */
int pebblegpu_siggen_set_sweep(pebblegpu_siggen *g, const pebblegpu_sweep *s);
int pebblegpu_siggen_set_noise(pebblegpu_siggen *g, double amplitude, uint64_t seed);
/* as pebblegpu_set_testbench_morse: replaces the set and restarts the stations only; generate then makes sweep + stations + noise */
int pebblegpu_siggen_set_morse(pebblegpu_siggen *g, const pebblegpu_morse_station *stations, uint32_t n_stations, int mix);
/* which stream of a receiver's noise this generator makes (default 0); does not reset */
int pebblegpu_siggen_set_stream(pebblegpu_siggen *g, uint32_t stream);
/* the next n samples into d_iq (device float2, in place: mixed with what is there, or replacing it); queues and returns */
int pebblegpu_siggen_generate_device(pebblegpu_siggen *g, void *d_iq, uint64_t n);
int pebblegpu_siggen_synchronize(pebblegpu_siggen *g);
/* TestBench::genSweep(n, iq) then TestBench::genNoise(n, iq) on a host frame of n CPX, in place; results are float-rounded */
int pebblegpu_siggen_generate(pebblegpu_siggen *g, double *iq, uint32_t n);
/* for parity checks: the accepted 31-bit draws (r [n][2]) and the accepted attempt's number (attempt [n]; 32: none) of noise samples
 * first_sample .. first_sample + n - 1 of the generator's stream with its current seed, computed on the device; host arrays */
int pebblegpu_siggen_noise_draws(pebblegpu_siggen *g, uint64_t first_sample, uint32_t n, uint32_t *r, uint8_t *attempt);

/* ------------------------------------------------------------------------------------------------
 * Host egress: the audio output stage and IQ recording through pinned slots.
 * The two steps the reference ends its chain with, as ONE mechanism -- the ingest slots in the other direction: a small packing
 * kernel is queued behind the process call on the call's own stream, its output travels on a copy stream into a ring of pinned host
 * slots, and the host waits for one slot's event, never for the device.  Without a ring the only way to a call's audio is
 * pebblegpu_receiver_audio + pebblegpu_receiver_synchronize / pebblegpu_memcpy_d2h, which drain the device after every call.
 *
 * Audio output: Receiver::processAudioData -> Audio::SendToOutput(in, n, m_gain, m_mute) (application/receiver.cpp:1029-1035; the sample
 * rule is pebblelib/audiopa.cpp:304-343, the same clip in pebblelib/audioqt.cpp:169-211), per selected channel:
 *     g = gain / 100.f;  t = a * g (ONE fp32 multiply: the reference's float(double(a) * double(g)), whose double product is exact);
 *     if (t > 0.9999f) t = 0.9999f; else if (t < -0.9999f) t = -0.9999f;        written interleaved L (real), R (imaginary)
 * The reference writes nothing when muted; a muted channel's row is zeros here.  NaN inputs: unpinned.  The source is the buffer
 * pebblegpu_receiver_audio reports -- the resampled audio when audio_rate is set, so the count can differ from call to call and is no
 * multiple of anything.  The reference's sound device takes floats: the two PCM16 formats are the library's own combination of that
 * clipped value with WavFile::WriteSamples' rule, (int16_t)((double)t * 32767), truncating (pebblelib/wavfile.cpp:387-388; the product
 * in double -- an fp32 product can round up to the next integer).
 *
 * ONE block per process call, always: call indices are 0-based from open and contiguous; a call that yields no audio (a one-channel
 * receiver's closed squelch, tune-only) gives a block with samples_per_channel == 0.  A FULL RING DROPS, IT DOES NOT REFUSE: when the
 * next slot has not been released as a call is queued, the call runs unchanged, its block is dropped and counted (the reference's
 * producer drops a frame the same way when no buffer is free; chain state never depends on the reader).  "Free" is host-side
 * bookkeeping only, so what is delivered and what is dropped does not depend on the device's timing.  n_slots: 2..8; 4 cover the
 * documented run-ahead of three calls.  Opening a ring changes no call's route or kernels (pebblegpu_receiver_kernel_name reports the
 * same strings): it adds one launch and one event to the call, and nothing the next call queues waits for the copy.  One reader, which
 * may run on another thread than the process calls; pebblegpu_process_iq / _process_iq_updates return their audio themselves and are
 * refused with PEBBLEGPU_E_UNSUPPORTED while a ring is open.  On the shard handles of a multibank (pebblegpu_multibank_shard) these
 * are setters and read-outs like any other: every shard has its own rings.
 * ---------------------------------------------------------------------------------------------- */
typedef enum {
    PEBBLEGPU_AUDIO_F32 = 0,      /* AudioPA::SendToOutput: float L, R interleaved, 8 bytes per sample */
    PEBBLEGPU_AUDIO_S16 = 1,      /* the same clipped value through WavFile::WriteSamples' rule, L, R, 4 bytes */
    PEBBLEGPU_AUDIO_S16_MONO = 2  /* left only, 2 bytes */
} pebblegpu_audio_format;
typedef struct {
    uint32_t struct_size;          /* = sizeof(pebblegpu_audio_block), set by the caller */
    uint32_t format;               /* pebblegpu_audio_format (a recording block: PEBBLEGPU_AUDIO_S16, left = I, right = Q) */
    uint64_t call_index;           /* which process call since open */
    const void *host;              /* pinned host memory: row r at host + r * pitch_bytes; NULL: no block (see _next) */
    uint64_t samples_per_channel;  /* may be 0 */
    uint64_t pitch_bytes;          /* a multiple of 16 */
    uint32_t n_channels;           /* rows: the selected channels (a recording block: the streams) */
    uint32_t dropped_before;       /* blocks dropped between the previous queued block and this one */
} pebblegpu_audio_block;
/* channels: row r of every block is channel channels[r] -- a subset, in any order; NULL: all n_channels of the receiver, in order
 * (n_channels is then ignored).  Duplicates, channels out of range, n_slots outside 2..8, an unknown format and a second open are
 * PEBBLEGPU_E_INVALID and leave the handle as it was. */
int pebblegpu_receiver_audio_out_open(pebblegpu_receiver *rx, int format, const uint32_t *channels, uint32_t n_channels, uint32_t n_slots);
/* waits for the handle's queued work, frees the ring (blocks not read are lost, and pointers handed out by _next become invalid).  A
 * reader that is inside _next on another thread is waited for (every copy is complete by then, so its wait ends); it returns
 * PEBBLEGPU_E_INVALID or its block, and must not touch the block after close returns */
int pebblegpu_receiver_audio_out_close(pebblegpu_receiver *rx);
/* Receiver::m_gain (the UI's 0..100; larger values amplify) and m_mute; defaults 100, 0.  gain must be finite and >= 0.  Takes effect at
 * the next process call like every setter (that call first waits for the calls before it: the rows' table is shared); kept while the
 * ring is closed. */
int pebblegpu_set_audio_level(pebblegpu_receiver *rx, uint32_t channel, float gain, int mute);
/* the oldest block not handed out yet.  wait != 0: blocks on that slot's event only.  b->host == NULL (and PEBBLEGPU_OK) when nothing
 * is queued, or with wait == 0 when the copy has not completed.  The memory stays valid until the block is released. */
int pebblegpu_receiver_audio_out_next(pebblegpu_receiver *rx, int wait, pebblegpu_audio_block *b);
/* gives the slot back: call_index must be the oldest handed-out block that has not been released, anything else is PEBBLEGPU_E_INVALID */
int pebblegpu_receiver_audio_out_release(pebblegpu_receiver *rx, uint64_t call_index);
int pebblegpu_receiver_audio_out_dropped(const pebblegpu_receiver *rx, uint64_t *blocks);   /* blocks dropped since open */
/* the host twin of the packing kernel (the same inline function; no device): n samples of interleaved float L, R -> out in `format` */
int pebblegpu_audio_out_convert(int format, float gain, int mute, const float *lr, uint64_t n, void *out);

/* IQ recording: if (m_isRecording) m_recordingFile.WriteSamples(nextStep, numSamples) (application/receiver.cpp:800-801), right behind
 * the test bench's injection: per call and stream the samples PEBBLEGPU_TAP_RAW_IQ shows -- after the generator, before the
 * conditioners (receiver.cpp:800-803) -- as PCM16 pairs, left = I, right = Q: the format PEBBLEGPU_IQ_WAV16 ingests.  Conversion:
 * (int16_t)((double)v * 32767), truncating (pebblelib/wavfile.cpp:377-396); where the reference's is undefined, |v * 32767| >= 32768,
 * the value saturates to +-32767; NaN gives 0.  A second ring of the same type, with the same block, drop and reader rules
 * (n_channels = streams, samples_per_channel = the call's n_samples, 4 bytes per sample).  On raw calls (pebblegpu_receiver_process_raw /
 * _process_ingested, multibank calls) with the test bench's generator off the kernel converts from the raw pairs itself, with
 * pebblegpu_normalize_iq's loader and scale, whether the call's own kernels convert in their loads (one channel beside the 8192-bin
 * transform: no float2 copy of the stream exists at all) or the call stages a converted copy for itself; the recording makes no
 * float2 copy of its own.  With the generator on, what the chain saw exists only in the buffer the generator wrote, and the kernel
 * reads that.  The kernel sits where the RAW_IQ tap's copy sits, and as with a tap a receiver without a
 * display transform runs its calls on ONE stream while a recording ring is open: recording is a diagnostic path, the audio ring is
 * the throughput path and has no such cost. */
int pebblegpu_receiver_record_open(pebblegpu_receiver *rx, uint32_t n_slots);
int pebblegpu_receiver_record_close(pebblegpu_receiver *rx);
int pebblegpu_receiver_record_next(pebblegpu_receiver *rx, int wait, pebblegpu_audio_block *b);
int pebblegpu_receiver_record_release(pebblegpu_receiver *rx, uint64_t call_index);
/* host twin: n IQ samples of interleaved float I, Q -> n PCM16 pairs */
int pebblegpu_iq_record_convert(const float *iq, uint64_t n, int16_t *out);

/* The modem hook ring: what a digital-modem plugin receives, for the host's own decoders (RTTY, PSK, WWV ...), without a synchronize.
 * Source: the narrow branch's per-channel rows right behind NoiseFilter::ProcessBlock and before the Morse decoder and AGC::processBlock
 * -- the block DigitalModemInterface::processBlock is handed at application/receiver.cpp:979-980, at the demodulator rate; exactly the
 * values PEBBLEGPU_TAP_MODEM shows.  READ-ONLY, as the library's Morse modem is: a plugin that alters the stream
 * (nextStep = processBlock(nextStep)) is out of scope; what the host does with a block never reaches the chain.
 *
 * One block per process call with the rows of the selected channels, every super-frame of the call one after the other
 * (samples_per_channel = n_superframes * samples_per_superframe).  ABSENT PAIRS: the reference returns before the hook when the squelch
 * is closed (receiver.cpp:962-965) and when the channel is dmNONE (:968-971), so a (channel, super-frame) that the bank's gate closed, or
 * whose channel is dmNONE in that call, is absent: its samples in the block are zeros and its flag is 0.  TRAILER: one byte per (block
 * row, super-frame of the call), present[r * n_superframes + j], 1 = present, padded to 16 bytes; the packing launch writes it at
 * host + n_channels * pitch_bytes and it travels inside the block's one copy.  A one-channel receiver's closed call (the squelch's
 * read-back gate, tune-only) gives a block with samples_per_channel == 0, n_superframes == 0 and present == NULL, like the audio ring.
 * Formats: PEBBLEGPU_AUDIO_F32 -- the float2 rows verbatim, I then Q (no gain, no clip); PEBBLEGPU_AUDIO_S16 -- PCM16 pairs by the
 * recording ring's rule (pebblegpu_iq_record_convert); PEBBLEGPU_AUDIO_S16_MONO is PEBBLEGPU_E_INVALID.
 *
 * The ring's rules are the audio ring's, word for word: ONE block per process call, call indices 0-based from open; A FULL RING DROPS
 * AND COUNTS, IT NEVER STALLS OR REFUSES; n_slots 2..8; one reader, on any thread; pebblegpu_process_iq is refused while the ring is
 * open; the shards of a multibank use their borrowed handles (pebblegpu_multibank_shard).  OPENING THE RING CHANGES NO CALL'S ROUTE AND
 * NO KERNEL: pebblegpu_receiver_kernel_name reports the same strings, two-stage calls stay two-stage, and audio, Morse events, S-meter
 * rows and spectra are bit for bit what they are without it; it adds one packing launch (k_modem_pack) and one event to a call, queued
 * between the noise filter and the AGC, and nothing the rest of the call queues waits for the copy.  Unlike the MODEM tap the ring runs
 * under a squelch threshold (a bank's per-channel gate included), with the Morse modem on, and with pebblegpu_set_spectrum_updates.
 * Refusals, each leaving the handle as it was: PEBBLEGPU_E_UNSUPPORTED on a WFM receiver (the hook is on the narrow branch);
 * PEBBLEGPU_E_INVALID for duplicate channels, channels out of range, an empty list, n_slots outside 2..8, a format other than the two
 * above, a second open. */
typedef struct {
    uint32_t struct_size;            /* = sizeof(pebblegpu_modem_block), set by the caller */
    uint32_t format;                 /* PEBBLEGPU_AUDIO_F32 or PEBBLEGPU_AUDIO_S16: I, Q pairs */
    uint64_t call_index;             /* which process call since open */
    const void *host;                /* pinned host memory: row r at host + r * pitch_bytes; NULL: no block (see _next) */
    uint64_t samples_per_channel;    /* n_superframes * samples_per_superframe; may be 0 */
    uint64_t pitch_bytes;            /* a multiple of 16 */
    uint32_t n_channels;             /* rows: the selected channels */
    uint32_t dropped_before;         /* blocks dropped between the previous queued block and this one */
    uint32_t rate;                   /* samples per second of the rows: the demodulator rate */
    uint32_t n_superframes;          /* super-frames of the call (0 in a block of 0 samples) */
    uint64_t samples_per_superframe; /* per channel */
    const uint8_t *present;          /* [n_channels][n_superframes], points into the slot behind the rows; NULL in a block of 0 samples */
} pebblegpu_modem_block;
/* channels: row r of every block is channel channels[r] -- a subset, in any order; NULL: all channels of the receiver, in order */
int pebblegpu_receiver_modem_out_open(pebblegpu_receiver *rx, int format, const uint32_t *channels, uint32_t n_channels, uint32_t n_slots);
int pebblegpu_receiver_modem_out_close(pebblegpu_receiver *rx);   /* as pebblegpu_receiver_audio_out_close */
int pebblegpu_receiver_modem_out_next(pebblegpu_receiver *rx, int wait, pebblegpu_modem_block *b);
int pebblegpu_receiver_modem_out_release(pebblegpu_receiver *rx, uint64_t call_index);
int pebblegpu_receiver_modem_out_dropped(const pebblegpu_receiver *rx, uint64_t *blocks);
/* The modem hook ring AT A MODEM RATE: the same ring, opened with a modem bandwidth and a minimum rate, delivers every selected channel's
 * rows already decimated on the device by the reference's own Decimator chain for those parameters --
 * Decimator::buildDecimationChain(demodulator rate, max_bw, min_rate), pebblelib/decimator.cpp:64-149 (vDSP path, merged stages
 * included), the first thing a modem plugin does with its block (Morse::setSampleRate, plugins/MorseDigitalModem/morse.cpp:174-193, and
 * the head of its processBlock, :778-782).  At (1000 Hz, 8000 Hz) on a 64 kHz bank an eighth of the bytes cross the link and the host's
 * modems start at their Goertzel, PLL or matched filter.  min_rate == 0: the reference's minDecimatedSampleRate (15000).
 * THE STREAM of one selected channel is what ONE Decimator object, fresh when the ring is opened (all histories zero), produces when it
 * is fed, in order, exactly the (channel, super-frame) pairs the ring delivers as present, and nothing else: over an ABSENT pair (a closed
 * gate, dmNONE -- zeros and flag 0, as above), over a one-channel receiver's closed call (its block of 0 samples) and over a block the
 * full ring DROPPED (dropped_before: it was never delivered) the channel's decimator state stands still, and the next present pair
 * continues from the last delivered one.  Retunes, band-pass changes and mode changes other than to or from dmNONE reset nothing (the
 * reference's modem is not told); close followed by open gives a fresh decimator.  THE BLOCK is pebblegpu_modem_block with the same
 * trailer, layout and host twins: samples_per_superframe = demodulator samples per super-frame / D, rate = (uint32_t)(int) of the chain's
 * achieved rate (the cast of morse.cpp:193: 39062.5 Hz with (1000, 8000) gives 4882), F32 rows the decimated float pairs, S16 rows
 * pebblegpu_iq_record_convert of those same floats.  An EMPTY CHAIN (min_rate at or above the demodulator rate, or no design fits:
 * decimator.cpp:155-160 copies) gives bit for bit the blocks of pebblegpu_receiver_modem_out_open.  _next, _release, _close and _dropped
 * are the functions above; one modem ring of either kind is open at a time, and everything said above about the ring stays true: one
 * block per call, a full ring drops and counts, read-only, no call's route and no other kernel changes.  One launch per call
 * (k_modem_rate_pack, where k_modem_pack is queued otherwise) carries tiles of every (row, super-frame) through the whole chain in LDS;
 * there is no per-stage state, only the last `lookback` delivered demodulator samples per row.
 * pebblegpu_modem_rate_plan (no device): the chain, its rates and its look-back for a demodulator rate and a super-frame, with the
 * refusals of the open, each of which leaves the handle as it was: PEBBLEGPU_E_UNSUPPORTED -- a WFM receiver (open only); a chain that
 * contains a CIC3 stage, e.g. (64000, 100, 8000) -> [(cic3, 2), (hb11, 4)]: the merged CIC3's two-sample form is not built here; more
 * than PEBBLEGPU_MODEM_RATE_MAX_STAGES stages; a chain whose smallest tile (4 outputs and the look-back) exceeds the kernel's 4096
 * samples of LDS.  PEBBLEGPU_E_SIZE -- the super-frame's demodulator samples are no multiple of D; a stage would receive fewer inputs
 * from one super-frame than it has taps (the reference drops samples unfiltered there, decimator.cpp:602-625); the look-back exceeds
 * one super-frame.  PEBBLEGPU_E_INVALID -- max_bw == 0, and everything pebblegpu_receiver_modem_out_open refuses.  Not built: modem
 * chains of the CDownConvert kind (SetDataRate, the WWV plugin's form), the hook on WFM, on the stream bank and on pebblegpu_process_iq,
 * a per-channel (max_bw, min_rate). */
#define PEBBLEGPU_MODEM_RATE_MAX_STAGES 16
typedef struct {
    uint32_t struct_size;            /* = sizeof(pebblegpu_modem_rate_info), set by the caller */
    uint32_t rate_int;               /* (uint32_t)(int)rate: what the blocks report */
    float rate;                      /* the chain's achieved rate (Decimator's float) */
    uint32_t total_decimation;       /* D */
    uint32_t n_stages;               /* 0: an empty chain, the plain ring */
    uint32_t lookback;               /* H = sum_j (taps_j - 1) * prod_{i<j} stride_i, in demodulator samples */
    uint64_t samples_per_superframe; /* of the blocks: the argument / D */
    uint32_t taps[PEBBLEGPU_MODEM_RATE_MAX_STAGES];
    uint32_t stride[PEBBLEGPU_MODEM_RATE_MAX_STAGES];   /* decimate-by of the stage, merged picks included */
} pebblegpu_modem_rate_info;
int pebblegpu_receiver_modem_out_open_rate(pebblegpu_receiver *rx, int format, const uint32_t *channels, uint32_t n_channels, uint32_t n_slots,
                                           uint32_t max_bw, uint32_t min_rate);
int pebblegpu_modem_rate_plan(uint32_t demod_rate, uint64_t samples_per_superframe, uint32_t max_bw, uint32_t min_rate, pebblegpu_modem_rate_info *out);
/* host twin of the packing kernel (no device): n IQ samples of interleaved float I, Q -> out in `format` (F32: copied; S16: the record twin) */
int pebblegpu_modem_out_convert(int format, const float *iq, uint64_t n, void *out);
/* a block's layout (no device), the function the producer and the reader use: the row pitch, and where the trailer of n_channels *
 * n_superframes flags starts and how many bytes (a multiple of 16) it takes */
int pebblegpu_modem_out_layout(int format, uint32_t n_channels, uint64_t samples_per_channel, uint32_t n_superframes, uint64_t *pitch_bytes,
                               uint64_t *trailer_offset, uint64_t *trailer_bytes);

/* ------------------------------------------------------------------------------------------------
 * Host egress for a stream bank: the band-passed IQ of selected streams and the display rows of the spectra a call computed, through
 * the same rings of pinned slots (above).  Without a ring the only way to a call's results is
 * pebblegpu_streambank_filtered / _spectrum / _map_spectrum + pebblegpu_streambank_synchronize + pebblegpu_memcpy_d2h, which drain the
 * device after every call; with the rings a host runs a bank from pinned slots in (pebblegpu_streambank_ingest_*) to pinned slots out
 * with no synchronize in its loop and a reader on another thread.
 *
 * Both rings follow the audio ring's rules word for word.  ONE block per accepted process call (_process, _process_raw,
 * _process_ingested), always: indices are 0-based from the ring's open and contiguous; a call that does not run the ring's producer
 * (`what` without bit 0 for the IQ ring, without bit 1 for the display ring, n_samples == 0) gives a block of 0 samples / 0 rows and
 * queues no copy; a refused call gives no block and does not advance the index.  A FULL RING DROPS, IT NEVER REFUSES AND NEVER STALLS:
 * the call runs unchanged, its block is dropped and counted (_dropped, dropped_before); "free" is host bookkeeping only, so what is
 * delivered does not depend on the device's timing, and the band-pass overlap, the spectrum's carried amplitudes and the update timer
 * never depend on the reader.  The packing kernel is queued on the bank's stream behind the call's end (behind the join when
 * PEBBLEGPU_SB_SIDE=1 put the band-pass on the second stream), ahead of the next call's kernels, which overwrite the buffers it reads;
 * the copy travels on the ring's own stream, and nothing the next call queues waits for it.  An open ring changes no route
 * (pebblegpu_streambank_kernel_name reports the same strings) and leaves pebblegpu_streambank_filtered / _spectrum / _map_spectrum /
 * _spectrum_frames unchanged: it adds one launch and one event per ring to a call, however many streams are selected (the selection is
 * a table on the device, written at open), and no float2 copy of anything.  One reader per ring, which may run on another thread;
 * _next(wait) blocks on that slot's event only; _release takes the oldest handed-out block; n_slots: 2..8.
 *
 * Refused at open with PEBBLEGPU_E_INVALID, leaving the handle as it was: duplicate or out-of-range streams (or an empty list), n_slots
 * outside 2..8, an unknown format, a second open of the same ring; for the display ring also a map the mappings refuse (x_pixels or
 * y_pixels <= 0, max_db == min_db), a missing map for the two mapped formats, and a bank created with spectrum_bins == 0.  With
 * PEBBLEGPU_E_SIZE: a ring whose slots would pin more than 1 GiB of host memory in total (pinned memory is a resource of the whole
 * machine: select fewer streams, a smaller max_rows, or set the update gate).  _close waits for the bank's queued work, then for a
 * reader that is inside _next on another thread, then frees the ring; pebblegpu_streambank_destroy closes open rings.
 * ---------------------------------------------------------------------------------------------- */
/* The IQ ring.  streams: row r of every block is stream streams[r] -- a subset in any order; NULL: all streams, in order (n_streams is
 * then ignored).  format: PEBBLEGPU_AUDIO_F32 -- the float2 rows of pebblegpu_streambank_filtered verbatim, I then Q (no gain and no
 * clip: this is not the audio stage); PEBBLEGPU_AUDIO_S16 -- PCM16 pairs by the recording ring's rule, WavFile::WriteSamples
 * (pebblelib/wavfile.cpp:377-396): (int16_t)((double)v * 32767), truncating, saturating to +-32767 where the reference's conversion is
 * undefined, NaN -> 0; pebblegpu_iq_record_convert is its host twin.  PEBBLEGPU_AUDIO_S16_MONO is refused.  Blocks: n_channels = the
 * selected streams, samples_per_channel = the call's n_samples. */
int pebblegpu_streambank_iq_out_open(pebblegpu_streambank *sb, int format, const uint32_t *streams, uint32_t n_streams, uint32_t n_slots);
int pebblegpu_streambank_iq_out_close(pebblegpu_streambank *sb);
int pebblegpu_streambank_iq_out_next(pebblegpu_streambank *sb, int wait, pebblegpu_audio_block *b);
int pebblegpu_streambank_iq_out_release(pebblegpu_streambank *sb, uint64_t call_index);
int pebblegpu_streambank_iq_out_dropped(const pebblegpu_streambank *sb, uint64_t *blocks);

/* The display ring.  The rows of a block are the spectrum rows ITS call computed for each selected stream: every frame of the call
 * without an update gate, the gate's selection (which may be empty) with pebblegpu_streambank_set_spectrum_updates, none for a call
 * without bit 1 of `what`.  A block never repeats a row of an earlier call: after a call that selected nothing the display keeps
 * showing what the host already has, and the block has 0 rows.  max_rows (0, or more than the bank's max_frames: max_frames) sizes the
 * slots; a call that computed more rows delivers the LAST max_rows of them (the latest row is what a display shows) and first_row
 * says where they start: max_rows = 1 is "the latest spectrum of every call".
 *   PEBBLEGPU_DISPLAY_DB_F32            the float dB rows of pebblegpu_streambank_spectrum, verbatim; map is ignored and may be NULL
 *   PEBBLEGPU_DISPLAY_PIXELS_I32        FFT::mapFFTToScreen (pebblelib/fft.cpp:400-534) of each row with map: the values
 *                                       pebblegpu_streambank_map_spectrum writes, bit for bit (one computation, see pebblegpu_screen_map)
 *   PEBBLEGPU_DISPLAY_WATERFALL_ARGB32  SpectrumWidget::drawWaterfall (application/spectrumwidget.cpp:1098-1118) on those pixels: pixel
 *                                       value v becomes m_spectrumColors[255 - v] as 0xFFRRGGBB -- QColor::setRgb (alpha 255) in QRgb
 *                                       layout.  Requires map->y_pixels == 255, the value every waterfall call site passes
 *                                       (spectrumwidget.cpp:1285-1293, 1302-1349); anything else is PEBBLEGPU_E_INVALID
 * The palette is the constructor's loop (spectrumwidget.cpp:97-113), integer arithmetic as written, with one deviation: the reference
 * allocates 255 entries, writes entry 255 and reads it for v = 0, both out of bounds; the library's table has 256 entries with entry
 * 255 = what the loop computes for i = 255. */
typedef enum {
    PEBBLEGPU_DISPLAY_DB_F32 = 0,
    PEBBLEGPU_DISPLAY_PIXELS_I32 = 1,
    PEBBLEGPU_DISPLAY_WATERFALL_ARGB32 = 2
} pebblegpu_display_format;
typedef struct {
    uint32_t struct_size;          /* = sizeof(pebblegpu_display_block), set by the caller */
    uint32_t format;               /* pebblegpu_display_format */
    uint64_t call_index;           /* which process call since open */
    const void *host;              /* row j of selected stream r at host + r * stream_pitch_bytes + j * row_pitch_bytes; NULL: no block */
    uint32_t rows_per_stream;      /* may be 0 */
    uint32_t first_row;            /* index, among the rows the call computed, of the block's row 0 */
    uint32_t row_elems;            /* bins (DB_F32) or x_pixels; 4 bytes each */
    uint32_t n_streams;            /* the selected streams */
    uint32_t dropped_before;       /* blocks dropped between the previous queued block and this one */
    uint32_t reserved;
    uint64_t row_pitch_bytes;      /* a multiple of 16 (x_pixels need not be a multiple of 4) */
    uint64_t stream_pitch_bytes;   /* rows_per_stream * row_pitch_bytes */
} pebblegpu_display_block;
int pebblegpu_streambank_display_open(pebblegpu_streambank *sb, int format, const pebblegpu_screen_map *map, const uint32_t *streams,
                                      uint32_t n_streams, uint32_t max_rows, uint32_t n_slots);
int pebblegpu_streambank_display_close(pebblegpu_streambank *sb);
int pebblegpu_streambank_display_next(pebblegpu_streambank *sb, int wait, pebblegpu_display_block *b);
int pebblegpu_streambank_display_release(pebblegpu_streambank *sb, uint64_t call_index);
int pebblegpu_streambank_display_dropped(const pebblegpu_streambank *sb, uint64_t *blocks);
/* host twin of the waterfall's colour rule (the same inline function the packing kernel runs; no device): n pixel values -> n
 * 0xFFRRGGBB words.  A pixel outside 0..255 is PEBBLEGPU_E_INVALID. */
int pebblegpu_waterfall_colors(const int32_t *pixels, uint64_t n, uint32_t *argb);

/* ------------------------------------------------------------------------------------------------
 * The receiver's display ring: what SpectrumWidget::newFftData (application/spectrumwidget.cpp:1169-1357) draws from, through the same
 * pinned slots as the audio.  Without it a host that wants a call's display rows calls pebblegpu_receiver_map_spectrum /
 * _map_zoom_spectrum, pebblegpu_receiver_synchronize and pebblegpu_memcpy_d2h, which drain the device after every call and throw away
 * the run-ahead the audio ring keeps.  A block has ONE OR TWO PANES -- newFftData's top and bottom panel -- and each pane names
 *   source    PEBBLEGPU_PANE_SPECTRUM: the unprocessed spectrum (pebblegpu_receiver_spectrum), rows per STREAM;
 *             PEBBLEGPU_PANE_ZOOM: the zoomed spectra (pebblegpu_receiver_zoom_spectrum), rows per CHANNEL
 *   format    pebblegpu_display_format, as for the stream bank's ring; DB_F32 ignores the geometry
 *   geometry  unprocessed source: `map` as pebblegpu_receiver_map_spectrum takes it (the top panel's zoomed-in range around the mixer is
 *             a start_freq / stop_freq pair).  Zoomed source: map.y_pixels, x_pixels, max_db, min_db with `zoom` and `mode_offset`
 *             (host array of the receiver's n_channels entries, indexed by channel; NULL: all 0) as pebblegpu_receiver_map_zoom_spectrum
 *             takes them: the edges are SignalSpectrum::mapFFTZoomedToScreen's, per channel; map.start_freq / stop_freq are ignored
 *   rows      row r of the pane is stream / channel rows[r] of its source -- a subset in any order; NULL: all of them, in order
 *   max_rows  0, or more than a call can compute: every row a call can compute
 * Pixels are pebblegpu_receiver_map_spectrum's / _map_zoom_spectrum's bit for bit (one computation, and each row's lanes add in the
 * order the map functions use for it); colours are pebblegpu_waterfall_colors of those pixels.
 *
 * The rules are the stream bank's display ring, word for word.  ONE block per accepted process call (_process, _process_raw,
 * _process_ingested, multibank calls through the shard handles: every shard has its own ring), indices 0-based from open and
 * contiguous; one slot holds all panes of a call (one copy, one event) and _next fills all the panes' blocks for the same call_index.
 * A pane holds the rows ITS CALL computed: every frame without a gate; the gate's selection under pebblegpu_set_spectrum_updates,
 * possibly 0 rows (the two sources have timers of their own, so the panes' row counts differ); 0 rows for a call that ran no such
 * transform.  A block never repeats an earlier call's row: the row pebblegpu_receiver_map_spectrum maps "as frame 0" after a call that
 * made none is for the pull interface only.  More rows than max_rows: the LAST max_rows, first_row says where they start.  A FULL
 * RING DROPS AND COUNTS, it never refuses and never stalls; "free" is host bookkeeping only.  One reader, possibly on another thread;
 * n_slots 2..8.  Opening the ring changes no call's route (pebblegpu_receiver_kernel_name reports the same strings, the audio has the
 * same bits): per call it adds one launch where both sources are complete on one stream (a call that joins its streams, a receiver
 * without side-by-side calls), one per pane on the stream that wrote its source otherwise (PEBBLEGPU_PIPELINE=1), however many
 * channels are selected -- selection and per-channel geometry are a table on the device, written at open and at _set_pane -- and
 * nothing the next call queues waits for the copy.  pebblegpu_process_iq / _process_iq_updates are refused with
 * PEBBLEGPU_E_UNSUPPORTED while the ring is open.  _close waits for queued work, then for a reader inside _next;
 * pebblegpu_receiver_destroy closes an open ring.
 *
 * Refused at open with PEBBLEGPU_E_INVALID, leaving the handle as it was: n_panes outside 1..2, an unknown source or format, a source
 * the receiver does not compute (spectrum_bins == 0 / hires_bins == 0), a duplicate, out-of-range or empty selection, n_slots outside
 * 2..8, a second open, a geometry the mappings refuse (x_pixels or y_pixels <= 0, max_db == min_db), a waterfall pane with
 * y_pixels != 255, a non-finite zoom.  With PEBBLEGPU_E_SIZE: slots that would pin more than 1 GiB of host memory in total.
 * ---------------------------------------------------------------------------------------------- */
typedef enum {
    PEBBLEGPU_PANE_SPECTRUM = 0,
    PEBBLEGPU_PANE_ZOOM = 1
} pebblegpu_pane_source;
typedef struct pebblegpu_display_pane {
    uint32_t struct_size;          /* = sizeof(pebblegpu_display_pane) */
    uint32_t source;               /* pebblegpu_pane_source */
    uint32_t format;               /* pebblegpu_display_format */
    uint32_t max_rows;
    pebblegpu_screen_map map;      /* struct_size set; ignored by DB_F32 */
    double zoom;                   /* zoomed source only */
    const int32_t *mode_offset;    /* zoomed source only: [n_channels] or NULL */
    const uint32_t *rows;          /* [n_rows] or NULL: all */
    uint32_t n_rows;
    uint32_t reserved[5];
} pebblegpu_display_pane;
#define PEBBLEGPU_DISPLAY_MAX_PANES 2
int pebblegpu_receiver_display_open(pebblegpu_receiver *rx, const pebblegpu_display_pane *panes, uint32_t n_panes, uint32_t n_slots);
int pebblegpu_receiver_display_close(pebblegpu_receiver *rx);
/* blocks: n_panes pebblegpu_display_block, struct_size set in each; blocks[p] is pane p of the same call (n_streams = the pane's selected
 * rows).  blocks[0].host == NULL (and PEBBLEGPU_OK): nothing queued, or (wait == 0) not copied yet.  A pane of 0 rows has a host pointer
 * all the same. */
int pebblegpu_receiver_display_next(pebblegpu_receiver *rx, int wait, pebblegpu_display_block *blocks);
int pebblegpu_receiver_display_release(pebblegpu_receiver *rx, uint64_t call_index);
int pebblegpu_receiver_display_dropped(const pebblegpu_receiver *rx, uint64_t *blocks);
/* A pane's plot geometry -- map, zoom, mode offsets: what a resize, a dB-range or a zoom change does in the GUI.  `geometry` is a whole
 * pane description (the one passed to _open with its map, zoom or mode_offset changed): source and format must be the pane's own
 * (anything else is PEBBLEGPU_E_INVALID), rows, n_rows and max_rows are not read -- the pane keeps its selection and its max_rows.
 * Takes effect at the next process call like every setter (that call first waits for the calls before it: the table is shared).  A
 * row wider than the slots were sized for at open is PEBBLEGPU_E_SIZE; the refusals of _open apply to the new geometry. */
int pebblegpu_receiver_display_set_pane(pebblegpu_receiver *rx, uint32_t pane, const pebblegpu_display_pane *geometry);

/* ------------------------------------------------------------------------------------------------
 * Auto-scale: SpectrumWidget::recalcScale (application/spectrumwidget.cpp:693-734), the plot range the reference draws with by default
 * (AutoScaleMax / AutoScaleMin are both true, application/settings.cpp:70-71), computed on the device so that a display ring's pixels
 * and colours follow the signal without the host pulling dB rows.  The rule, for one unprocessed-spectrum row of `bins` float dB values
 * (each widened to double):
 *   pwr_i = pow(10, dB_i / 10.0) (DB::dBToPower);  total = sum pwr_i;  peak = max pwr_i (from 0);  avg = total / bins
 *   min_db = qBound(-120, ((int)(powerTodB(avg)  - 10) / 5) * 5, -70)      powerTodB(0) = -120, else 10 log10; (int) truncates; C division
 *   max_db = qBound( -50, ((int)(powerTodB(peak) + 10) / 5) * 5,   0)
 * The host twin (pebblegpu_auto_scale_row) is the reference's serial loop; the device (k_scale_stats: one 256-lane workgroup per row, a
 * fixed reduction order, no atomics -- the same bits on every run) adds in another order, so avg_power agrees to ~bins * 2^-53 relative
 * and a row whose powerTodB(avg) - 10 or powerTodB(peak) + 10 lies within that of an integer may come out 5 dB away.
 *
 * Pull interface: the scale of frames first_frame + j * frame_step (j < n_frames) of the LAST call's unprocessed spectrum, every
 * stream, into the device buffer d_out [stream][n_frames]; queued where pebblegpu_*_map_spectrum queues its map, results complete
 * after _synchronize; the same frame rules and refusals.
 *
 * The rings.  _display_set_auto_scale(flags) is maxDbChanged / minDbChanged with or without "Auto" (spectrumwidget.cpp:933-966);
 * _display_rescale is m_scaleNeedsRecalc = true (power-on :239, an LO change :562).  Both are HOST FLAGS consumed when the next call is
 * queued: they never wait for earlier calls (pebblegpu_receiver_display_set_pane does).
 *   - A flag that goes on requests a recalc; until it has happened the pane's own map.max_db / min_db hold for that end of the range
 *     (m_fullScaleDb / m_baseScaleDb).  A flag that goes off returns its end to the pane's map from the next call on.
 *   - The recalc happens in the first call after the request that computes at least one unprocessed-spectrum row, on that call's FIRST
 *     computed row of every stream ("wait for next fft to have new data", :1184-1187); a call under the update gate that computes none
 *     leaves it pending.  The new range maps every row of that call's block and of later blocks, in every mapped pane: a zoomed row takes
 *     the range of its channel's stream (stream 0 off a shared input) -- m_plotMaxDb / m_plotMinDb are the widget's.  DB_F32 panes ignore
 *     the range as they ignore the geometry.  The stream bank: stream s's rows are mapped with stream s's range.
 *   - Cost: one launch (k_scale_stats, a workgroup per stream) in the recalc call, ahead of the packing launch -- and, where that call's
 *     two pipelines end on different streams (PEBBLEGPU_PIPELINE=1), two event records and two waits that order the table's write against
 *     the other stream -- and nothing in any other call: the packing kernels read the range once per row from a table on the device, and
 *     a call that computed no row queues nothing, as before.  With flags 0 blocks, launches and pebblegpu_*_kernel_name strings are
 *     exactly as without this interface.
 *   - While a flag is on every block THAT HAS ROWS carries, behind its rows and inside the slot's one copy, the ranges it was mapped with:
 *     one pebblegpu_display_scale per selected stream (a receiver: per selected row of pane 0, by the row's stream), read with
 *     _display_scale for a block that is currently handed out (PEBBLEGPU_E_INVALID for any other call_index, for a block queued while the
 *     flags were 0 and for a block without a row of any pane: it maps nothing, the ranges of the last block with rows still hold).
 *     An end whose flag is off reports the pane's (pane 0's; the stream bank: the map's) own value, truncated to int.  avg_power /
 *     peak_power are those of the recalc in the block's own call and 0 in every other block.
 * Refused with PEBBLEGPU_E_INVALID, the handle left as it was: no open ring; unknown flag bits; a receiver without an unprocessed spectrum
 * (spectrum_bins == 0); a stream bank ring in DB_F32 (nothing is mapped); MAX alone with a mapped pane whose fixed min_db >= -50, MIN
 * alone with one whose fixed max_db <= -70 (the range could come out empty or upside down), and a later _set_pane that would create either.
 * "Alone" is judged twice: by the flags, and by the ends the table supplies at that moment -- a flag whose recalc is still pending leaves
 * its end to the pane, so with MAX in use and MIN just requested a fixed min_db >= -50 is refused until the recalc has landed.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t max_db, min_db;        /* m_plotMaxDb, m_plotMinDb */
    double avg_power, peak_power;  /* avgPwr, peakPwr of the row the range came from */
} pebblegpu_display_scale;
#define PEBBLEGPU_AUTO_SCALE_MAX 1
#define PEBBLEGPU_AUTO_SCALE_MIN 2
/* host twin (no device): recalcScale's loop over one row, serial as the reference */
int pebblegpu_auto_scale_row(const float *db, uint32_t bins, pebblegpu_display_scale *out);
int pebblegpu_receiver_spectrum_scale(pebblegpu_receiver *rx, uint32_t first_frame, uint32_t n_frames, uint32_t frame_step,
                                      pebblegpu_display_scale *d_out);
int pebblegpu_streambank_spectrum_scale(pebblegpu_streambank *sb, uint32_t first_frame, uint32_t n_frames, uint32_t frame_step,
                                        pebblegpu_display_scale *d_out);
int pebblegpu_receiver_display_set_auto_scale(pebblegpu_receiver *rx, uint32_t flags);
int pebblegpu_receiver_display_rescale(pebblegpu_receiver *rx);
/* out: cap entries; *n = the entries written */
int pebblegpu_receiver_display_scale(pebblegpu_receiver *rx, uint64_t call_index, pebblegpu_display_scale *out, uint32_t cap, uint32_t *n);
int pebblegpu_streambank_display_set_auto_scale(pebblegpu_streambank *sb, uint32_t flags);
int pebblegpu_streambank_display_rescale(pebblegpu_streambank *sb);
int pebblegpu_streambank_display_scale(pebblegpu_streambank *sb, uint64_t call_index, pebblegpu_display_scale *out, uint32_t cap, uint32_t *n);

/* ------------------------------------------------------------------------------------------------
 * Stream bank: per-stream S-meter and squelch-gated IQ blocks.  The reference's order in Receiver::processIQData is band-pass, then
 * SignalStrength::fdEstimate (application/signalstrength.cpp:287-380) on the unprocessed spectrum over the band-pass window, then the
 * squelch return (application/receiver.cpp:950-965); the bank runs the last two on the device, so a host that watches many streams
 * neither pulls dB rows nor ships the IQ of streams that carry nothing.
 *
 * The rule, for one row of `bins` float dB values (each widened to double): binWidth = sample_rate / bins (INTEGER division);
 *   mixerBin = qBound(0, (int)(bins / 2 + mixer_freq / binWidth), bins);   lo / hi = qBound(0, (int)(mixerBin + bp_lo|bp_hi / binWidth), bins)
 *   bpBins = hi - lo;   noiseLow = qBound(0, lo - bpBins, bins);   noiseHigh = qBound(0, hi + bpBins, bins)
 *   over i in [noiseLow, min(noiseHigh, bins - 1)]: pwr = pow(10, dB_i / 10.0); lo <= i <= hi: total += pwr, peak = max; else noise += pwr
 *   peakDb = clip(powerTodB(peak)); avgDb = clip(powerTodB(total / bpBins)); floorDb = clip(powerTodB(noise / noiseBins));
 *   snrDb = bound(0, 10 log10(peak / noiseAvg), 120), 0 when either is 0.      powerTodB(0) = -120; clip bounds to -120..0
 * clip and bound are the reference's qBound(lo, v, hi) = qMax(lo, qMin(hi, v)), whose comparisons are all false for a NaN: a NaN comes out
 * as the LOWER bound.  So bpBins == 0 with a bin in band gives avgDb 0 (x / 0 = inf); a window without a noise bin (0 / 0) floorDb -120 and
 * snrDb 0; a window without any bin (the mixer's bin clamped to `bins`) (-120, -120, 0, -120).  No output is ever NaN or infinite.
 * pebblegpu_signal_strength_row is the host twin (no device): the reference's serial loop; out = (peakDb, avgDb, snrDb, floorDb).
 * PEBBLEGPU_E_INVALID for a NULL argument, 0 bins, or sample_rate < bins (the integer bin width would be 0).  The device
 * (k_stream_strength: one 256-lane workgroup per row, a fixed reduction order, no atomics -- the same bits on every run) adds in another
 * order: the four values agree with the twin's on the same row to ~1e-4 dB.
 *
 * _enable_signal_strength(sb, on): from the next call on every call that computes unprocessed-spectrum rows queues ONE more launch behind
 * its end (behind the join with PEBBLEGPU_SB_SIDE=1), whether or not a ring is open; a call that computes no row launches nothing.
 * Stream s's window is its own band-pass (lo, hi) as float -- what the last ACCEPTED pebblegpu_streambank_set_bandpass left; (-1, 1),
 * CFastFIR's constructor state, before the first -- around mixer frequency 0 at the bank's sample_rate rounded to whole Hz.  Needs
 * spectrum_bins != 0 and a bin width of at least 1 Hz (else PEBBLEGPU_E_INVALID).  Off cannot be chosen while a stream's squelch is above
 * -120 (PEBBLEGPU_E_INVALID).  With the S-meter off a call queues exactly what it queued before this interface existed.
 * _signal_strength(sb, &rows_per_stream, &pitch): a device pointer to float4 [stream][pitch] (peakDb, avgDb, snrDb, floorDb), one entry per
 * row the LAST call computed, indexed like pebblegpu_streambank_spectrum -- under the update gate the computed rows only, possibly none;
 * complete after pebblegpu_streambank_synchronize.  NULL and 0 rows while the S-meter is off.
 *
 * _set_squelch(sb, stream, squelch_db): one threshold per stream, narrowed to float; -120 and below never closes (the default).  A
 * threshold above -120 turns the S-meter on (and is refused where that is).  PEBBLEGPU_E_INVALID: stream out of range, a non-finite value.
 * The setters are HOST STATE consumed when the next call is queued: tables are uploaded in stream order from pinned staging, no call waits
 * for the calls before it.  The decision is per (stream, frame of cfg.frame samples -- processIQData's buffer), made on the device with
 * no read-back: closed = avgDb < squelch_db on the float the S-meter reported.  The row frame f reads (getUnprocessed(), receiver.cpp:959-965):
 * its own when the call computed one for f; else the latest computed at or before f, carried from an earlier call if need be (a call
 * without bit 1 of `what` reads the carried one); before any row exists (since the S-meter went on) the gate is open.
 * What the gate suppresses is what lies behind the band-pass: the IQ ring.  A closed (stream, frame) is zeros in the block (0.0f pairs in
 * F32, 0 pairs in S16), an open one bit for bit what the ring delivered before.  pebblegpu_streambank_filtered is in FRONT of the gate, as
 * the band-pass is in the reference: its bits, the overlap and the spectrum never depend on a threshold.  The rows go through the gated
 * instance of the packing kernel only while some threshold is above -120.
 *
 * The trailer.  While the S-meter is on every IQ block THAT HAS SAMPLES carries, behind its rows and inside the slot's one copy, one
 * pebblegpu_stream_gate per (selected stream r, frame j of the call), entry r * n_frames + j: the values the frame's decision read, `open`,
 * and `row` -- the computed-row index of this call they came from, PEBBLEGPU_GATE_ROW_CARRIED (an earlier call's) or
 * PEBBLEGPU_GATE_ROW_NONE (none yet: values 0, open 1).  _iq_out_gate reads it for a block that is currently handed out (out: cap entries;
 * *n_frames = the call's frames): PEBBLEGPU_E_INVALID for any other call_index and for a block queued while the S-meter was off or without
 * samples, PEBBLEGPU_E_SIZE when n_selected * n_frames entries do not fit cap.  Every IQ ring reserves n_selected * max_frames entries per
 * slot at open (counted in the 1 GiB limit) whether or not the S-meter is on: 24 bytes per (stream, frame) of pinned memory that an
 * S-meter that stays off never copies.
 * ---------------------------------------------------------------------------------------------- */
typedef struct pebblegpu_stream_gate {
    float peak_db, avg_db, snr_db, floor_db;
    uint32_t open;                 /* 0: the frame is zeros in the block */
    uint32_t row;
} pebblegpu_stream_gate;
#define PEBBLEGPU_GATE_ROW_CARRIED 0xFFFFFFFEu
#define PEBBLEGPU_GATE_ROW_NONE 0xFFFFFFFFu
int pebblegpu_signal_strength_row(const float *db, uint32_t bins, uint32_t sample_rate, float bp_lo, float bp_hi, double mixer_freq, float out[4]);
int pebblegpu_streambank_enable_signal_strength(pebblegpu_streambank *sb, int on);
const void *pebblegpu_streambank_signal_strength(const pebblegpu_streambank *sb, uint64_t *rows_per_stream, uint64_t *pitch);
int pebblegpu_streambank_set_squelch(pebblegpu_streambank *sb, uint32_t stream, double squelch_db);
int pebblegpu_streambank_iq_out_gate(pebblegpu_streambank *sb, uint64_t call_index, pebblegpu_stream_gate *out, uint32_t cap, uint32_t *n_frames);

/* ------------------------------------------------------------------------------------------------
 * Stream bank: input conditioners.  The four steps Receiver::processIQData runs ahead of both of the bank's transforms
 * (application/receiver.cpp:814-823): DCRemoval, IQBalance, NoiseBlanker::ProcessBlock, NoiseBlanker::ProcessBlock2 -- in that order,
 * per stream, all default-off.  flags: PEBBLEGPU_COND_* or'ed, as for pebblegpu_set_conditioners.
 *
 * _set_conditioners(sb, stream, flags, iq_gain, iq_phase) is HOST STATE consumed when the next call is queued: it touches no device
 * memory and makes no device or stream synchronisation (the receivers' setter does; a bank runs from pinned slots with no synchronise in
 * its loop).  The next conditioned call uploads the table from pinned staging in stream order.  Switching NB1 on resets its magnitude
 * average and spike count, switching NB2 on its two averages (setNbEnabled / setNb2Enabled, noiseblanker.cpp:20-37), on the device, in
 * stream order ahead of that call; NB1's delay line and the DC filter's state carry on.  A blanker that is off leaves its state alone (its
 * averages start at 1, the constructor's value).  PEBBLEGPU_E_INVALID, handle usable afterwards: a NULL handle, a stream out of range,
 * flags outside 0..15, a non-finite gain or phase.
 *
 * While ANY stream has a flag set every call with n > 0 conditions its samples first, whatever `what` asks for: the state advances with
 * the sample stream.  The caller's input is never written: the first pass over it is out of place, into a float2 buffer the bank owns
 * ([n_streams][capacity], allocated by the first conditioned call together with the state; a second one when NB1 is on, shared with the
 * normalised copy of staged raw calls); streams with flags 0 are copied by that pass, bit for bit.  The band-pass, the display transform
 * and with them the S-meter, the squelch gate, _map_spectrum and both rings read the conditioned rows.  A raw call is staged:
 * k_normalize_iq, the conditioners, the float2 kernels (pebblegpu_streambank_kernel_name: "k_normalize_iq + k_condition + <the float2
 * route>"; a float2 call: "k_condition + <route>"); raw and float2 calls still continue each other.  pebblegpu_streambank_last_ms which 0
 * and 1 include the conditioners.  With no flag ever set, or all cleared again, a call queues exactly what it queued before this
 * interface existed: the same routes, names and bits.
 * IQBalance restarts its adaptive terms every cfg.frame samples (the reference's numSamples).
 *
 * _conditioned(sb, &samples_per_stream, &pitch_samples): a device pointer to float2 [stream][pitch], the rows the LAST call's transforms
 * read; valid until the next call, complete after pebblegpu_streambank_synchronize.  NULL and 0 when the last call conditioned nothing.
 *
 * The kernels (csrc/kernels_condition.h) are parallel in time: a stream's call is cut into chunks of 2048 samples, one workgroup each.
 * Per stage: every chunk's contribution from a zero entry state, a fixed-order scan of those per stream, then every chunk again from its
 * true entry state.  Every reduction has a fixed order: the same call sequence gives the same bits.  Against the serial form:
 *   DC removal: fp64 state as there; a chunk's entry state is M^2048 applied to the one before plus the chunk's zero-state end state
 *     instead of 2048 sequential steps -- another fp64 rounding order, far below the float the samples are stored in.  No warm-up; the
 *     state carried between calls is the last chunk's end state.
 *   NB1 / NB2 magnitude averages, a <- (float)(0.999 a + 0.001 mag): every run of 8 samples takes its entry value from the fp64
 *     recurrence (rounded to float once) and then rounds per step as the reference does.  The serial float chain drifts from the exact
 *     recurrence by about 2e-6 relative, this form by at most 8 roundings: the averages agree to the last bits, NOT bit for bit, and a
 *     blanker decision mag > 3.3 avg that lies within those bits can fall the other way.  So can the same samples cut into other calls.
 *   NB2's complex average (pole 0.75, fp64 in the reference too): entry values from the same scan; its value is used rounded to float.
 *   NB1's spike count: exact (maps on the 8 counts, composed in order).  Its output is the input two samples earlier (DelayLine(8, 2));
 *     the two samples in front of a call are carried state.
 *   IQBalance: the reference's arithmetic step by step, one workgroup per (stream, frame).
 * ---------------------------------------------------------------------------------------------- */
int pebblegpu_streambank_set_conditioners(pebblegpu_streambank *sb, uint32_t stream, int flags, double iq_gain, double iq_phase);
const void *pebblegpu_streambank_conditioned(const pebblegpu_streambank *sb, uint64_t *samples_per_stream, uint64_t *pitch_samples);

#ifdef __cplusplus
}
#endif
#endif /* PEBBLEGPU_H */
