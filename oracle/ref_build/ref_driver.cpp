/* ref_driver -- runs the reference's own DSP classes (compiled unmodified from the reference tree) on a file of
 * float64 input and writes what they produce.  It restates no arithmetic: constructors and methods only.
 *
 *   ref_driver STAGE IN OUT [numbers...]
 *
 * IN:  raw float64, interleaved (re, im) unless the stage says otherwise.
 * OUT: raw float64 records, each [count, count values]; complex values are interleaved.
 * The stages and their arguments are listed in main(); tests/reference_cases.py is the other end of this interface.
 *
 * Private members are read (coefficients, clocks, chain tables) by compiling this one file with the access
 * keywords opened; the reference's sources are compiled as they are.
 */
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>
#include "qt_standins.h"

#define private public
#define protected public
#include "cpx.h"
#include "mixer.h"
#include "decimator.h"
#include "downconvert.h"
#include "fastfir.h"
#include "fft.h"
#include "fftaccelerate.h"
#include "fftooura.h"
#include "fir.h"
#include "iir.h"
#include "fractresampler.h"
#include "global.h"
#include "agc.h"
#include "noiseblanker.h"
#include "noisefilter.h"
#include "dcremoval.h"
#include "iqbalance.h"
#include "signalstrength.h"
#include "goertzel.h"
#include "movingavgfilter.h"
#include "sampleclock.h"
#include "demod_am.h"
#include "demod_sam.h"
#include "demod_nfm.h"
#include "demod_wfm.h"
#include "morse.h"
#include "morsegen.h"
#undef private
#undef protected

Global *global = nullptr;
/* what moc would generate for the one signal the driven classes declare */
void SignalStrength::newSignalStrength(double, double, double, double, double) {}
/* The base class of the four demodulators lives in the application's demod.cpp, which brings the GUI with it.  The demodulators use
 * nothing of it but its constructor and destructor; these two are this project's text, written from the declarations in demod.h (the
 * destructor is the class's key function, so the vtable and the typeinfo come with it) */
Demod::Demod(quint32 r, quint32 n) : ProcessStep(r, n) {}
Demod::~Demod() {}

static std::vector<double> g_in;
static FILE *g_out;
static std::vector<double> g_arg;

static void rec(const double *v, size_t n)
{
    double c = double(n);
    fwrite(&c, sizeof c, 1, g_out);
    if (n)
        fwrite(v, sizeof(double), n, g_out);
}
static void rec1(double v) { rec(&v, 1); }
static void rec_cpx(const CPX *v, size_t n) { rec(reinterpret_cast<const double *>(v), 2 * n); }
static CPX *in_cpx() { return reinterpret_cast<CPX *>(g_in.data()); }
static size_t in_len() { return g_in.size() / 2; }
static double arg(size_t i)
{
    if (i >= g_arg.size()) {
        fprintf(stderr, "ref_driver: missing argument %zu\n", i);
        exit(2);
    }
    return g_arg[i];
}

/* mixer FS N F0 [RETUNE_FRAME F1]: one record per frame */
static void st_mixer()
{
    quint32 n = quint32(arg(1));
    Mixer m(quint32(arg(0)), n);
    m.setFrequency(arg(2));
    for (size_t f = 0; f * n + n <= in_len(); f++) {
        if (g_arg.size() > 4 && f == size_t(arg(3)))
            m.setFrequency(arg(4));
        rec_cpx(m.processBlock(in_cpx() + f * n), n);
    }
}

/* decimator FS BW N PLAIN: records: rate, decBy2Stages, chain (taps, stride pairs), then one record per frame.
 * PLAIN=1 runs the chain through HalfbandFilter::process (no vDSP) */
static void st_decimator()
{
    quint32 n = quint32(arg(2));
    Decimator d(quint32(arg(0)), n);
    if (arg(3) != 0)
        d.m_useVdsp = false;
    rec1(d.buildDecimationChain(quint32(arg(0)), quint32(arg(1))));
    rec1(d.decBy2Stages());
    std::vector<double> chain;
    for (int i = 0; i < d.m_decimationChain.length(); i++) {
        HalfbandFilter *h = d.m_decimationChain[i];
        chain.push_back(h->m_useCIC3 ? 0 : h->m_numTaps);
        chain.push_back(h->m_decimate);
    }
    rec(chain.data(), chain.size());
    std::vector<CPX> out(n + 16);
    for (size_t f = 0; f * n + n <= in_len(); f++) {
        quint32 k = d.process(in_cpx() + f * n, out.data(), n);
        rec_cpx(out.data(), k);
    }
    if (arg(3) != 0)
        d.m_useVdsp = true; /* the destructor frees what the constructor made */
}

/* downconvert INRATE MAXBW SIMPLE (LEN FREQ CWOFFSET)...: records: rate, then one record per call; the setters are
 * called before a call whose frequency or offset differs from the call before */
static void st_downconvert()
{
    CDownConvert d;
    double rate = arg(2) != 0 ? d.SetDataRateSimple(arg(0), arg(1)) : d.SetDataRate(arg(0), arg(1));
    rec1(rate);
    size_t pos = 0;
    double pf = 0, pc = 0;
    for (size_t c = 0; 3 + 3 * c + 2 < g_arg.size(); c++) {
        int n = int(g_arg[3 + 3 * c]);
        double f = g_arg[4 + 3 * c], cw = g_arg[5 + 3 * c];
        if (c == 0 || f != pf || cw != pc) {
            d.SetCwOffset(cw);
            d.SetFrequency(f);
        }
        pf = f;
        pc = cw;
        std::vector<CPX> work(in_cpx() + pos, in_cpx() + pos + n), out(n + 16); /* ProcessData mixes its input in place */
        int k = d.ProcessData(n, work.data(), out.data());
        rec_cpx(out.data(), k);
        pos += n;
    }
}

/* fastfir LO HI OFFSET FS N: records: H (2048 complex), then one record per block */
static void st_fastfir()
{
    CFastFIR f;
    int n = int(arg(4));
    f.SetupParameters(arg(0), arg(1), arg(2), arg(3));
    rec_cpx(f.m_pFilterCoef, f.m_Fft->getFFTSize());
    std::vector<CPX> out(in_len() + 4 * 8192);
    for (size_t b = 0; b * n + n <= in_len(); b++) {
        int k = f.ProcessData(n, in_cpx() + b * n, out.data());
        rec_cpx(out.data(), k);
    }
}

/* fir NTAPS SCALE ASTOP FPASS FSTOP FS: records: tap count, taps, filtered input */
static void st_fir()
{
    CFir f;
    int nt = f.InitLPFilter(int(arg(0)), arg(1), arg(2), arg(3), arg(4), arg(5));
    rec1(nt);
    rec(f.m_Coef, nt);
    std::vector<CPX> out(in_len());
    f.ProcessFilter(int(in_len()), in_cpx(), out.data());
    rec_cpx(out.data(), out.size());
}

/* iir KIND(0 LP, 1 HP) F0 Q FS: records: (b0 b1 b2 a1 a2), filtered input */
static void st_iir()
{
    CIir q;
    if (arg(0) == 0)
        q.InitLP(arg(1), arg(2), arg(3));
    else
        q.InitHP(arg(1), arg(2), arg(3));
    double c[5] = {q.m_B0, q.m_B1, q.m_B2, q.m_A1, q.m_A2};
    rec(c, 5);
    std::vector<CPX> out(in_len());
    q.ProcessFilter(int(in_len()), in_cpx(), out.data());
    rec_cpx(out.data(), out.size());
}

/* resampler MAXIN RATE N: per frame two records: output, m_FloatTime */
static void st_resampler()
{
    CFractResampler r;
    int n = int(arg(2));
    r.Init(int(arg(0)));
    std::vector<CPX> out(size_t(n / arg(1)) + 16);
    for (size_t f = 0; f * n + n <= in_len(); f++) {
        int k = r.Resample(n, arg(1), in_cpx() + f * n, out.data());
        rec_cpx(out.data(), k);
        rec1(r.m_FloatTime);
    }
}

/* spectrum FFTSIZE SPB FS OOURA LEN...: per frame two records: dB bins, overload flag.  The previous-frame
 * buffers are uninitialised in the reference; they are zeroed here so that frame 0 is defined */
static void st_spectrum()
{
    FFT *f = arg(3) != 0 ? static_cast<FFT *>(new FFTOoura()) : FFT::factory("ref_driver");
    f->fftParams(quint32(arg(0)), 0, arg(2), int(arg(1)), WindowFunction::BLACKMANHARRIS);
    int bins = f->getFFTSize();
    memset(f->m_fftPower, 0, bins * sizeof(double));
    memset(f->m_fftAmplitude, 0, bins * sizeof(double));
    memset(f->m_fftPhase, 0, bins * sizeof(double));
    std::vector<double> out(bins);
    size_t pos = 0;
    for (size_t i = 4; i < g_arg.size(); i++) {
        int n = int(g_arg[i]);
        bool over = f->fftSpectrum(in_cpx() + pos, out.data(), n);
        pos += n;
        rec(out.data(), bins);
        rec1(over ? 1 : 0);
    }
    delete f;
}

/* mapscreen FFTSIZE FS Y X MAXDB MINDB START STOP: IN is one dB row of FFTSIZE real doubles; the FFT is made as in the spectrum stage
 * (a buffer of FFTSIZE samples), then FFT::mapFFTToScreen of IN; one record, the X pixels */
static void st_mapscreen()
{
    FFT *f = FFT::factory("ref_driver");
    f->fftParams(quint32(arg(0)), 0, arg(1), int(arg(0)), WindowFunction::BLACKMANHARRIS);
    if (g_in.size() != size_t(f->getFFTSize())) {
        fprintf(stderr, "ref_driver: mapscreen wants %d values\n", f->getFFTSize());
        exit(2);
    }
    int x = int(arg(3));
    std::vector<qint32> px(x > 0 ? x : 1);
    f->mapFFTToScreen(g_in.data(), qint32(arg(2)), qint32(x), arg(4), arg(5), qint32(arg(6)), qint32(arg(7)), px.data());
    std::vector<double> out(px.begin(), px.begin() + (x > 0 ? x : 0));
    rec(out.data(), out.size());
    delete f;
}

/* agc FS N (MODE THRESHOLD)...: one block per pair, setAgcMode when the pair changes; one record per block */
static void st_agc()
{
    quint32 n = quint32(arg(1));
    AGC a(quint32(arg(0)), n);
    double pm = -1, pt = -1;
    for (size_t b = 0; 2 + 2 * b + 1 < g_arg.size(); b++) {
        double m = g_arg[2 + 2 * b], t = g_arg[3 + 2 * b];
        if (m != pm || t != pt)
            a.setAgcMode(AGC::AgcMode(int(m)), int(t));
        pm = m;
        pt = t;
        rec_cpx(a.processBlock(in_cpx() + b * n), n);
    }
}

/* nb WHICH(1|2) FS N ON...: one block per flag; the setter is called when the flag changes; one record per block */
static void st_nb()
{
    quint32 n = quint32(arg(2));
    NoiseBlanker nb(quint32(arg(1)), n);
    int which = int(arg(0)), prev = 0;
    for (size_t b = 0; 3 + b < g_arg.size(); b++) {
        int on = int(g_arg[3 + b]);
        if (on != prev) {
            if (which == 1)
                nb.setNbEnabled(on != 0);
            else
                nb.setNb2Enabled(on != 0);
        }
        prev = on;
        CPX *o = which == 1 ? nb.ProcessBlock(in_cpx() + b * n) : nb.ProcessBlock2(in_cpx() + b * n);
        rec_cpx(o, n);
    }
}

/* anf FS N: one record per block */
static void st_anf()
{
    quint32 n = quint32(arg(1));
    NoiseFilter nf(quint32(arg(0)), n);
    nf.enableStep(true);
    for (size_t b = 0; b * n + n <= in_len(); b++)
        rec_cpx(nf.ProcessBlock(in_cpx() + b * n), n);
}

/* iqbalance FS N GAIN PHASE: one record per block */
static void st_iqbalance()
{
    quint32 n = quint32(arg(1));
    IQBalance q(quint32(arg(0)), n);
    q.enableStep(true);
    q.setAutomatic(false);
    q.setGainFactor(arg(2));
    q.setPhaseFactor(arg(3));
    for (size_t b = 0; b * n + n <= in_len(); b++)
        rec_cpx(q.ProcessBlock(in_cpx() + b * n), n);
}

/* dcremoval FS N: one record per block */
static void st_dcremoval()
{
    quint32 n = quint32(arg(1));
    DCRemoval d(quint32(arg(0)), n);
    d.enableStep(true);
    for (size_t b = 0; b * n + n <= in_len(); b++)
        rec_cpx(d.process(in_cpx() + b * n, n), n);
}

/* fdestimate FS N RATE MIXER (LO HI)...: IN is one dB spectrum (real doubles); one record (peak, avg, snr, floor,
 * returned value) per band */
static void st_fdestimate()
{
    SignalStrength s(quint32(arg(0)), quint32(arg(1)));
    for (size_t b = 0; 4 + 2 * b + 1 < g_arg.size(); b++) {
        double r = s.fdEstimate(g_in.data(), int(g_in.size()), quint32(arg(2)), float(g_arg[4 + 2 * b]), float(g_arg[5 + 2 * b]), arg(3));
        double v[5] = {s.peakDb(), s.avgDb(), s.snrDb(), s.floorDb(), r};
        rec(v, 5);
    }
}

/* goertzel RATE FRAMES N FREQ [SWITCH_AT FREQ2]: GoertzelOOK the way the Morse modem drives it (morse.cpp:228-232, :345-373,
 * :861-866): constructed, its rate set, TH_PEAK (the constructor's own choice, said again), setFreq(freq, N, jitterCount), then
 * processSample(CPX, ...) on every sample;
 * setFreq again before sample SWITCH_AT (Morse::setDemodMode on a running modem).  Records: powers, decisions, peak powers, one
 * value per result, then the samples left in the block under way */
static void st_goertzel()
{
    quint32 rate = quint32(arg(0)), n = quint32(arg(2));
    GoertzelOOK g(rate, quint32(arg(1)));
    g.setTargetSampleRate(rate);
    g.setThresholdType(GoertzelOOK::TH_PEAK);
    int jitter = int(rate * .005 / n);
    g.setFreq(int(arg(3)), n, jitter);
    std::vector<double> pw, above, peak;
    for (size_t i = 0; i < in_len(); i++) {
        if (g_arg.size() > 5 && i == size_t(arg(4)))
            g.setFreq(int(arg(5)), n, jitter);
        double p = 0, pk = 0;
        bool a = false;
        if (g.processSample(in_cpx()[i], p, a, pk)) {
            pw.push_back(p);
            above.push_back(a ? 1 : 0);
            peak.push_back(pk);
        }
    }
    rec(pw.data(), pw.size());
    rec(above.data(), above.size());
    rec(peak.data(), peak.size());
    rec1(g.m_mainTone.m_nCount);
}

/* sampleclock RATE (EARLIER LATER)...: one record, SampleClock::uSecDelta of every pair; IN is not read */
static void st_sampleclock()
{
    SampleClock c(quint32(arg(0)));
    c.reset();
    std::vector<double> out;
    for (size_t i = 1; i + 1 < g_arg.size(); i += 2)
        out.push_back(c.uSecDelta(quint32(g_arg[i]), quint32(g_arg[i + 1])));
    rec(out.data(), out.size());
}

/* movingavg LEN RESET_AT: IN is real doubles; MovingAvgFilter(LEN)::newSample of each, reset() before sample RESET_AT; one record */
static void st_movingavg()
{
    MovingAvgFilter f(quint32(arg(0)));
    std::vector<double> out;
    for (size_t i = 0; i < g_in.size(); i++) {
        if (i == size_t(arg(1)))
            f.reset();
        out.push_back(f.newSample(g_in[i]));
    }
    rec(out.data(), out.size());
}

/* ---- the Morse modem plugin (plugins/MorseDigitalModem/morse.cpp, compiled as it is).  Its signals are plain member calls here (emit
 * is empty, nothing is connected), and their bodies, which moc would generate, are this driver's observation points ---- */
static struct {
    quint32 samples; /* modem samples since the last setSampleRate: one testbench(CPX) per sample, morse.cpp:887 */
    std::vector<double> powers, tones, events, stars;
} g_morse;

void Morse::testbench(int, CPX *buf, double, int)
{
    g_morse.samples++;
    /* Goertzel::processSample leaves its count at 0 exactly where it returned a result (goertzel.cpp:253) */
    if (m_goertzel->m_mainTone.m_nCount == 0) {
        g_morse.powers.push_back(m_goertzel->m_mainTone.m_power); /* not m_testBenchValue's, which is times 100 */
        g_morse.tones.push_back(buf->imag() != 0 ? 1 : 0);
    }
}
void Morse::testbench(int, double *, double, int) {}
bool Morse::addProfile(QString, int) { return true; }
void Morse::removeProfile(quint16) {}
/* outputString has appended to m_output; the dot-dash buffer is still whole (resetDotDashBuf follows, morse.cpp:1081-1083).  The sample
 * under way has not been counted yet (stateMachine runs before testbench).  One event: sample, token, kind (0 character, 1 word
 * space); stars: the numbers of the events for which the plugin printed '*' (a token that is no character) */
void Morse::newOutput()
{
    bool word = m_output.s.size() >= 1 && m_output.s.back() == ' ' && m_dotDashBufIndex == 0;
    g_morse.events.push_back(double(g_morse.samples + 1));
    g_morse.events.push_back(word ? 0.0 : double(m_morseCode.tokenizeDotDash(m_dotDashBuf)));
    g_morse.events.push_back(word ? 1.0 : 0.0);
    if (!m_output.s.empty() && m_output.s.back() == '*')
        g_morse.stars.push_back(double(g_morse.events.size() / 3 - 1));
}

static void morse_status(Morse *m, std::vector<double> &out)
{
    double v[10] = {double(m->m_wpmSpeedCurrent), double(m->m_aboveWpmRange), double(m->m_belowWpmRange), double(m->m_modemSampleRate),
                    double(m->m_goertzelSamplesPerResult), double(m->m_usecDotDashThreshold), double(m->m_usecElementThreshold),
                    double(m->m_usecCharThreshold), double(m->m_usecWordThreshold), double(m->m_usecShortestMark)};
    out.insert(out.end(), v, v + 10);
}

/* morse RATE FRAME WPM0 OUTMODE (AT ACT)...: Morse(), setSampleRate(RATE, FRAME), then processBlock frame by frame.  Before the frame
 * that starts at input sample AT: ACT 0 = setSampleRate(RATE, FRAME) again, otherwise setDemodMode(ACT) (8 dmCWL, 9 dmCWU); several
 * pairs may name one AT and run in their order.  ACT < 0 takes a status and does nothing else.  OUTMODE is written to m_outputMode behind every
 * setSampleRate (init sets CHAR_ONLY).
 * The constructor leaves m_wpmSpeedCurrent, the two range limits and the state unset and setSampleRate reads them (morse.cpp:240,
 * :671-684, :588): the object is built over zeroed memory, m_wpmSpeedCurrent is WPM0 and the limits are the class's own defaults,
 * which init assigns a few lines after reading them -- what every later setSampleRate finds there.
 * Records: decisions, events (3 values each), stars, statuses (10 values: one before every ACT <= 0 and one at the end), powers */
static void st_morse()
{
    int rate = int(arg(0)), n = int(arg(1));
    void *mem = calloc(1, sizeof(Morse));
    Morse *m = new (mem) Morse();
    m->m_wpmSpeedCurrent = int(arg(2));
    m->m_wpmLimitLow = m->c_wpmLowDefault;
    m->m_wpmLimitHigh = m->c_wpmHighDefault;
    m->setSampleRate(rate, n);
    m->m_outputMode = Morse::OUTPUT_MODE(int(arg(3)));
    g_morse.samples = 0;
    std::vector<double> status;
    for (size_t f = 0; f * n + n <= in_len(); f++) {
        for (size_t i = 4; i + 1 < g_arg.size(); i += 2) {
            if (size_t(g_arg[i]) != f * n)
                continue;
            int act = int(g_arg[i + 1]);
            if (act <= 0)
                morse_status(m, status);
            if (act == 0) {
                m->setSampleRate(rate, n);
                m->m_outputMode = Morse::OUTPUT_MODE(int(arg(3)));
                g_morse.samples = 0;
            } else if (act > 0)
                m->setDemodMode(DeviceInterface::DemodMode(act));
        }
        m->processBlock(in_cpx() + f * n);
    }
    morse_status(m, status);
    rec(g_morse.tones.data(), g_morse.tones.size());
    rec(g_morse.events.data(), g_morse.events.size());
    rec(g_morse.stars.data(), g_morse.stars.size());
    rec(status.data(), status.size());
    rec(g_morse.powers.data(), g_morse.powers.size());
    /* the plugin's destructor frees what memalign gave and deletes the rest; the process ends here instead */
}

/* morsegen RATE FREQ DB WPM RISE N CHAR...: MorseGen(RATE), setParams(FREQ, DB, WPM, RISE), setTextOut(the CHARs, byte values), then
 * nextOutputSample N times.  Records: (rise, fall, dot, dot buffer, dash, dash buffer, element, character, word) sample counts, then
 * the N samples */
static void st_morsegen()
{
    MorseGen g(arg(0));
    g.setParams(arg(1), arg(2), quint32(arg(3)), quint32(arg(4)));
    QString text;
    for (size_t i = 6; i < g_arg.size(); i++)
        text.s.push_back(char(int(g_arg[i])));
    g.setTextOut(text);
    double c[9] = {double(g.m_numSamplesRise), double(g.m_numSamplesFall), double(g.m_numSamplesDot), double(g.m_numSamplesDotBuf),
                   double(g.m_numSamplesDash), double(g.m_numSamplesDashBuf), double(g.m_numSamplesElementBuf),
                   double(g.m_numSamplesCharBuf), double(g.m_numSamplesWordBuf)};
    rec(c, 9);
    std::vector<CPX> out(size_t(arg(5)));
    for (size_t i = 0; i < out.size(); i++)
        out[i] = g.nextOutputSample();
    rec_cpx(out.data(), out.size());
}

/* The call scripts of the demodulator stages: the lengths from argument FIRST on (with STEP arguments per call); a call never exceeds
 * the buffer size the class was constructed with, nor PHZBUF_SIZE for WFM */
static int call_len(size_t i, quint32 n, size_t pos)
{
    int len = int(g_arg[i]);
    if (len < 0 || quint32(len) > n || len > PHZBUF_SIZE || pos + size_t(len) > in_len()) {
        fprintf(stderr, "ref_driver: call of %d samples at %zu (buffer %u, input %zu)\n", len, pos, n, in_len());
        exit(2);
    }
    return len;
}

/* demod_am FS N (LEN BW)...: Demod::processBlock's dmAM (demod.cpp:104-107): setBandwidth where BW != 0, then processBlockFiltered;
 * one record per call */
static void st_demod_am()
{
    quint32 n = quint32(arg(1));
    Demod_AM d(int(arg(0)), int(n));
    std::vector<CPX> out(n);
    size_t pos = 0;
    for (size_t i = 2; i + 1 < g_arg.size(); i += 2) {
        int len = call_len(i, n, pos);
        if (g_arg[i + 1] != 0)
            d.setBandwidth(g_arg[i + 1]);
        d.processBlockFiltered(in_cpx() + pos, out.data(), len);
        rec_cpx(out.data(), size_t(len));
        pos += size_t(len);
    }
}

/* demod_sam FS N LEN...: dmSAM (demod.cpp:108-110), Demod_SAM::processBlock; one record per call */
static void st_demod_sam()
{
    quint32 n = quint32(arg(1));
    Demod_SAM d(int(arg(0)), int(n));
    std::vector<CPX> out(n);
    size_t pos = 0;
    for (size_t i = 2; i < g_arg.size(); i++) {
        int len = call_len(i, n, pos);
        d.processBlock(in_cpx() + pos, out.data(), len);
        rec_cpx(out.data(), size_t(len));
        pos += size_t(len);
    }
}

/* demod_nfm FS N LEN...: dmFMN (demod.cpp:111-115), Demod_NFM::processBlockNCO; one record per call */
static void st_demod_nfm()
{
    quint32 n = quint32(arg(1));
    Demod_NFM d(int(arg(0)), int(n));
    std::vector<CPX> out(n);
    size_t pos = 0;
    for (size_t i = 2; i < g_arg.size(); i++) {
        int len = call_len(i, n, pos);
        d.processBlockNCO(in_cpx() + pos, out.data(), len);
        rec_cpx(out.data(), size_t(len));
        pos += size_t(len);
    }
}

/* Demod_WFM leaves m_RdsLastData (and its work arrays) uninitialised; it is constructed over zeroed memory here so that the first
 * bit decision is defined */
static Demod_WFM *new_wfm(int fs, int n)
{
    void *mem = calloc(1, sizeof(Demod_WFM));
    return new (mem) Demod_WFM(fs, n);
}
static void delete_wfm(Demod_WFM *d)
{
    d->~Demod_WFM();
    free(d);
}

/* demod_wfm_mono FS N LEN...: Demod::fmMono (demod.cpp:169-175), processDataMono, which filters its input in place; per call two
 * records: the returned count, the output */
static void st_demod_wfm_mono()
{
    quint32 n = quint32(arg(1));
    Demod_WFM *d = new_wfm(int(arg(0)), int(n));
    std::vector<CPX> out(n);
    size_t pos = 0;
    for (size_t i = 2; i < g_arg.size(); i++) {
        int len = call_len(i, n, pos);
        std::vector<CPX> work(in_cpx() + pos, in_cpx() + pos + len);
        int k = d->processDataMono(len, work.data(), out.data());
        rec1(k);
        rec_cpx(out.data(), size_t(k));
        pos += size_t(len);
    }
    delete_wfm(d);
}

/* demod_wfm_stereo FS N LEN...: Demod::fmStereo (demod.cpp:198-226): processDataStereo (its input buffer is its scratch), then
 * getStereoLock, then ONE getNextRdsGroupData; per call four records: the returned count, the output, (changed, lock), (got, BlockA,
 * BlockB, BlockC, BlockD).  After the last call the queue is drained into one more record, four words per group */
static void st_demod_wfm_stereo()
{
    quint32 n = quint32(arg(1));
    Demod_WFM *d = new_wfm(int(arg(0)), int(n));
    std::vector<CPX> out(n);
    size_t pos = 0;
    for (size_t i = 2; i < g_arg.size(); i++) {
        int len = call_len(i, n, pos);
        std::vector<CPX> work(in_cpx() + pos, in_cpx() + pos + len);
        int k = d->processDataStereo(len, work.data(), out.data());
        rec1(k);
        rec_cpx(out.data(), size_t(k));
        int lock = 0;
        int changed = d->getStereoLock(&lock);
        double lk[2] = {double(changed), double(lock)};
        rec(lk, 2);
        tRDS_GROUPS g = {0, 0, 0, 0};
        int got = d->getNextRdsGroupData(&g); /* 0 for an empty queue (the words stay 0) and for a group equal to the one before */
        double gr[5] = {double(got), double(g.BlockA), double(g.BlockB), double(g.BlockC), double(g.BlockD)};
        rec(gr, 5);
        pos += size_t(len);
    }
    std::vector<double> rest;
    while (d->m_RdsQHead != d->m_RdsQTail) {
        tRDS_GROUPS g = {0, 0, 0, 0};
        d->getNextRdsGroupData(&g);
        rest.push_back(g.BlockA);
        rest.push_back(g.BlockB);
        rest.push_back(g.BlockC);
        rest.push_back(g.BlockD);
    }
    rec(rest.data(), rest.size());
    delete_wfm(d);
}

int main(int argc, char **argv)
{
    static const struct { const char *name; void (*fn)(); } stages[] = {
        {"mixer", st_mixer}, {"decimator", st_decimator}, {"downconvert", st_downconvert}, {"fastfir", st_fastfir},
        {"fir", st_fir}, {"iir", st_iir}, {"resampler", st_resampler}, {"spectrum", st_spectrum}, {"mapscreen", st_mapscreen}, {"agc", st_agc},
        {"nb", st_nb}, {"anf", st_anf}, {"iqbalance", st_iqbalance}, {"dcremoval", st_dcremoval}, {"fdestimate", st_fdestimate},
        {"goertzel", st_goertzel}, {"sampleclock", st_sampleclock}, {"movingavg", st_movingavg}, {"demod_am", st_demod_am},
        {"demod_sam", st_demod_sam}, {"demod_nfm", st_demod_nfm}, {"demod_wfm_mono", st_demod_wfm_mono},
        {"demod_wfm_stereo", st_demod_wfm_stereo}, {"morse", st_morse}, {"morsegen", st_morsegen}};
    if (argc < 4) {
        fprintf(stderr, "usage: ref_driver STAGE IN OUT [numbers...]\n");
        return 2;
    }
    FILE *fi = fopen(argv[2], "rb");
    if (!fi) {
        perror(argv[2]);
        return 2;
    }
    fseek(fi, 0, SEEK_END);
    long bytes = ftell(fi);
    fseek(fi, 0, SEEK_SET);
    g_in.resize(size_t(bytes) / sizeof(double) + 2);
    if (bytes && fread(g_in.data(), 1, size_t(bytes), fi) != size_t(bytes)) {
        perror("read");
        return 2;
    }
    g_in.resize(size_t(bytes) / sizeof(double));
    fclose(fi);
    for (int i = 4; i < argc; i++)
        g_arg.push_back(strtod(argv[i], nullptr));
    g_out = fopen(argv[3], "wb");
    if (!g_out) {
        perror(argv[3]);
        return 2;
    }
    for (const auto &s : stages)
        if (!strcmp(argv[1], s.name)) {
            s.fn();
            return fclose(g_out) ? 2 : 0;
        }
    fprintf(stderr, "ref_driver: unknown stage %s\n", argv[1]);
    return 2;
}
