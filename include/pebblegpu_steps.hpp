// pebblegpu_steps.hpp -- header-only C++ adapters over the C ABI (pebblegpu.h) with the reference's own
// call shapes, so application/receiver.cpp could swap these classes in for pebblelib's, plus a Qt-free
// stand-in for the FileSDRDevice plugin that feeds any CB_ProcessIQData-shaped callback from an IQ .wav.
//
//   reference interface                                                 adapter here
//   ------------------------------------------------------------------  -----------------------------------
//   using CPX = std::complex<double>            pebblelib/cpx.h:96       pebblegpu::CPX
//   CPX *ProcessStep::process(CPX*, quint32)    application/processstep.h:24   ProcessStep::process
//   CPX *Mixer::processBlock(CPX*) / setFrequency   pebblelib/mixer.h:15-16    Mixer
//   float Decimator::buildDecimationChain / quint32 process / decBy2Stages
//                                               pebblelib/decimator.h:236-239  Decimator
//   void CFastFIR::SetupParameters / int ProcessData    pebblelib/fastfir.h:57-59  CFastFIR
//   BandPassFilter::setBandPass / process       application/bandpassfilter.h    BandPassFilter
//   CPX *Demod::processBlock(CPX*, int) / setDemodMode / setBandwidth
//                                               application/demod.h:33-40       Demod
//   FFT::fftParams / bool fftSpectrum(CPX*, double*, int) / bool mapFFTToScreen(...)   pebblelib/fft.h:30-56   FFT
//   WindowFunction::WINDOWTYPE                  pebblelib/windowfunction.h:10-11   WindowFunction
//   bool SignalSpectrum::mapFFTToScreen(...)    application/signalspectrum.cpp:137-149   Receiver::mapFFTToScreen
//   void Receiver::processIQData(CPX*, quint16) application/receiver.cpp:758    Receiver::processIQData
//   CB_ProcessIQData / CB_ProcessAudioData      pebblelib/device_interfaces.h:32,38   same std::function shapes
//   void TestBench::genSweep(int, CPX*) / genNoise(int, CPX*)   application/testbench.h; NCO::initSweep pebblelib/nco.h:52-57   TestBench
//   void MorseGen::setParams(double, double, quint32, quint32) / setTextOut / nextOutputSample   plugins/MorseGenDevice/morsegen.h   MorseGen
//   FileSDRDevice (initialize / Cmd_Start pump) plugins/FileSDRDevice/filesdrdevice.cpp:24-33,226-289   FileSdrFeeder
//
// Error behaviour follows the reference: no exceptions across step calls; a failing call logs to stderr (the
// reference uses qDebug) and returns the input pointer / zero count; lastStatus() exposes the C status code.
#ifndef PEBBLEGPU_STEPS_HPP
#define PEBBLEGPU_STEPS_HPP
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "pebblegpu.h"

namespace pebblegpu {

using CPX = std::complex<double>;
static_assert(sizeof(CPX) == 2 * sizeof(double), "CPX must be interleaved doubles");

typedef std::function<void(CPX *, uint16_t)> CB_ProcessIQData;     // device_interfaces.h:32
typedef std::function<void(CPX *, uint16_t)> CB_ProcessAudioData;  // device_interfaces.h:38

enum DemodMode { dmAM = 0, dmSAM, dmFMN, dmFMM, dmFMS, dmDSB, dmLSB, dmUSB, dmCWL, dmCWU, dmDIGL, dmDIGU, dmNONE };  // :124-138

inline int report(const char *what, int rc)
{
    if (rc != 0) std::fprintf(stderr, "pebblegpu: %s failed (%d): %s\n", what, rc, pebblegpu_last_error());
    return rc;
}

// application/processstep.{h,cpp}: owns nothing here (the library owns the buffers); keeps the enable flag contract
class ProcessStep {
public:
    ProcessStep(uint32_t sampleRate_, uint32_t bufferSize_) : sampleRate(sampleRate_), numSamples(bufferSize_), bufferSize(bufferSize_) {}
    virtual ~ProcessStep() {}
    virtual CPX *process(CPX *in, uint32_t) { return in; }
    uint32_t getSampleRate() const { return sampleRate; }
    uint32_t getBufferSize() const { return bufferSize; }
    void enableStep(bool e) { enabled = e; }
    bool isEnabled() const { return enabled; }
    int lastStatus() const { return status; }

protected:
    uint32_t sampleRate, numSamples, bufferSize;
    bool enabled = false;
    int status = 0;
};

class Mixer {
public:
    Mixer(uint32_t sampleRate, uint32_t bufferSize, int device = 0) { status = report("mixer_create", pebblegpu_mixer_create(device, sampleRate, bufferSize, &h)); }
    ~Mixer() { pebblegpu_mixer_destroy(h); }
    Mixer(const Mixer &) = delete;
    Mixer &operator=(const Mixer &) = delete;
    void setFrequency(double f) { if (h) status = report("mixer_set_frequency", pebblegpu_mixer_set_frequency(h, f)); }
    CPX *processBlock(CPX *in)
    {
        const double *out = nullptr;
        if (!h || (status = report("mixer_process", pebblegpu_mixer_process(h, reinterpret_cast<const double *>(in), &out))) != 0) return in;
        return reinterpret_cast<CPX *>(const_cast<double *>(out));
    }
    int lastStatus() const { return status; }

private:
    pebblegpu_mixer *h = nullptr;
    int status = 0;
};

class Decimator {
public:
    Decimator(uint32_t sampleRate, uint32_t bufferSize, int device = 0) { status = report("decimator_create", pebblegpu_decimator_create(device, sampleRate, bufferSize, &h)); }
    ~Decimator() { pebblegpu_decimator_destroy(h); }
    Decimator(const Decimator &) = delete;
    Decimator &operator=(const Decimator &) = delete;
    float buildDecimationChain(uint32_t sampleRateIn, uint32_t protectBw, uint32_t sampleRateOut = 0)
    {
        float r = (float)sampleRateIn;
        if (h) status = report("decimator_build_chain", pebblegpu_decimator_build_chain(h, sampleRateIn, protectBw, sampleRateOut, &r));
        return r;
    }
    uint32_t process(CPX *in, CPX *out, uint32_t numSamples)
    {
        uint32_t n = 0;
        if (!h) return 0;
        status = report("decimator_process", pebblegpu_decimator_process(h, reinterpret_cast<const double *>(in), reinterpret_cast<double *>(out), numSamples, &n));
        return status ? 0 : n;
    }
    uint32_t decBy2Stages()
    {
        uint32_t s = 0;
        if (h) pebblegpu_decimator_dec_by2_stages(h, &s);
        return s;
    }
    int lastStatus() const { return status; }

private:
    pebblegpu_decimator *h = nullptr;
    int status = 0;
};

// CDownConvert (pebblelib/downconvert.h:25-50): same member names and argument meaning; TYPECPX = CPX
class CDownConvert {
public:
    explicit CDownConvert(uint32_t maxInLength = 65536, int device = 0) { status = report("downconvert_create", pebblegpu_downconvert_create(device, maxInLength, &h)); }
    ~CDownConvert() { pebblegpu_downconvert_destroy(h); }
    CDownConvert(const CDownConvert &) = delete;
    CDownConvert &operator=(const CDownConvert &) = delete;
    void SetFrequency(double NcoFreq) { if (h) status = report("downconvert_set_frequency", pebblegpu_downconvert_set_frequency(h, NcoFreq)); }
    void SetCwOffset(double offset) { if (h) status = report("downconvert_set_cw_offset", pebblegpu_downconvert_set_cw_offset(h, offset)); }
    double SetDataRate(double InRate, double MaxBW)
    {
        double r = InRate;
        if (h) status = report("downconvert_set_data_rate", pebblegpu_downconvert_set_data_rate(h, InRate, MaxBW, 0, &r));
        return r;
    }
    double SetDataRateSimple(double InRate, double MaxBW)
    {
        double r = InRate;
        if (h) status = report("downconvert_set_data_rate", pebblegpu_downconvert_set_data_rate(h, InRate, MaxBW, 1, &r));
        return r;
    }
    // returns the number of samples written to pOutData; pInData is left as it was (the reference mixes it in place)
    int ProcessData(int InLength, CPX *pInData, CPX *pOutData)
    {
        uint32_t n = 0;
        if (!h || InLength <= 0) return 0;
        status = report("downconvert_process", pebblegpu_downconvert_process(h, (uint32_t)InLength, reinterpret_cast<const double *>(pInData), reinterpret_cast<double *>(pOutData), &n));
        return status ? 0 : (int)n;
    }
    int lastStatus() const { return status; }

private:
    pebblegpu_downconvert *h = nullptr;
    int status = 0;
};

class CFastFIR {
public:
    explicit CFastFIR(uint32_t fftSize = 0, uint32_t firSize = 0, int device = 0) { status = report("fastfir_create", pebblegpu_fastfir_create(device, fftSize, firSize, &h)); }
    ~CFastFIR() { pebblegpu_fastfir_destroy(h); }
    CFastFIR(const CFastFIR &) = delete;
    CFastFIR &operator=(const CFastFIR &) = delete;
    void SetupParameters(double FLoCut, double FHiCut, double Offset, double SampleRate)
    {
        if (!h) return;
        status = pebblegpu_fastfir_setup(h, FLoCut, FHiCut, Offset, SampleRate);
        if (status == PEBBLEGPU_E_FILTER_PARAM) std::fprintf(stderr, "Filter Parameter error\n");  // fastfir.cpp:214
        else report("fastfir_setup", status);
    }
    int ProcessData(int InLength, CPX *InBuf, CPX *OutBuf)
    {
        int n = 0;
        if (!h) return 0;
        status = report("fastfir_process", pebblegpu_fastfir_process(h, InLength, reinterpret_cast<const double *>(InBuf), reinterpret_cast<double *>(OutBuf), &n));
        return status ? 0 : n;
    }
    int lastStatus() const { return status; }

private:
    pebblegpu_fastfir *h = nullptr;
    int status = 0;
};

// application/bandpassfilter.{h,cpp} with m_useFastFIR = true
class BandPassFilter : public ProcessStep {
public:
    BandPassFilter(uint32_t sampleRate_, uint32_t bufferSize_, int device = 0) : ProcessStep(sampleRate_, bufferSize_), fir(0, 0, device), out(bufferSize_ + 2048) {}
    void setBandPass(float low, float high)
    {
        lowFreq_ = low;
        highFreq_ = high;
        fir.SetupParameters(low, high, 0, sampleRate);  // bandpassfilter.cpp:43
    }
    CPX *process(CPX *in, uint32_t n) override
    {
        fir.ProcessData((int)n, in, out.data());  // the count is ignored, as in bandpassfilter.cpp:53-56
        status = fir.lastStatus();
        return out.data();
    }
    float lowFreq() const { return lowFreq_; }
    float highFreq() const { return highFreq_; }

private:
    CFastFIR fir;
    std::vector<CPX> out;
    float lowFreq_ = 0, highFreq_ = 0;
};

class Demod : public ProcessStep {
public:
    Demod(uint32_t sampleRate_, uint32_t wfmSampleRate, uint32_t bufferSize_, int device = 0) : ProcessStep(sampleRate_, bufferSize_)
    {
        status = report("demod_create", pebblegpu_demod_create(device, sampleRate_, wfmSampleRate, bufferSize_, &h));
    }
    ~Demod() override { pebblegpu_demod_destroy(h); }
    Demod(const Demod &) = delete;
    Demod &operator=(const Demod &) = delete;
    void setDemodMode(DemodMode m, int /*sourceSampleRate*/ = 0, int /*audioSampleRate*/ = 0)
    {
        mode = m;
        if (h) status = report("demod_set_mode", pebblegpu_demod_set_mode(h, (int)m));
    }
    DemodMode demodMode() const { return mode; }
    void setBandwidth(double bw) { if (h) status = report("demod_set_bandwidth", pebblegpu_demod_set_bandwidth(h, bw)); }
    CPX *processBlock(CPX *in, int bufSize)
    {
        const double *out = nullptr;
        if (!h || (status = report("demod_process", pebblegpu_demod_process(h, reinterpret_cast<const double *>(in), bufSize, &out))) != 0) return in;
        return reinterpret_cast<CPX *>(const_cast<double *>(out));
    }
    // int Demod_WFM::getNextRdsGroupData(tRDS_GROUPS *), demod_wfm.h:39, as Demod::fmStereo calls it (demod.cpp:207-219: once behind
    // every processDataStereo): 0 while nothing is queued or the group repeats the one before it, else 1 with the group in *g -- the
    // value to hand to CRdsDecode::decodeRdsGroup when BlockA != 0.  (The library has popped one group per processBlock call already;
    // this walks that list.)
    int getStereoLock(int *pPilotLock)  // Demod_WFM::getStereoLock, demod_wfm.h:40
    {
        int lock = 0, changed = 0;
        if (!h || pebblegpu_demod_stereo_lock(h, &lock, &changed) != 0) return 0;
        if (pPilotLock) *pPilotLock = lock;
        return changed;
    }
    int getNextRdsGroupData(pebblegpu_rds_group *g)
    {
        uint32_t n = 0;
        uint8_t changed = 0;
        if (!h || !g || pebblegpu_demod_rds_groups(h, g, &changed, 1, &n) != 0 || n == 0) return 0;
        return changed ? 1 : 0;
    }

private:
    pebblegpu_demod *h = nullptr;
    DemodMode mode = dmAM;
};

// pebblelib/windowfunction.h:10-11: the window types FFT::fftParams takes, with the reference's numeric values
class WindowFunction {
public:
    enum WINDOWTYPE { RECTANGULAR = 1, HANNING, WELCH, PARZEN, BARTLETT, HAMMING, BLACKMAN2, BLACKMAN3, BLACKMAN4, EXPONENTIAL, RIEMANN,
                      BLACKMANHARRIS, BLACKMAN, NONE };
};

// pebblelib/fft.h as SignalSpectrum uses it (factory + fftParams + fftSpectrum + mapFFTToScreen); window type is BLACKMANHARRIS
class FFT {
public:
    explicit FFT(int device_ = 0) : device(device_) {}
    ~FFT() { pebblegpu_spectrum_destroy(h); }
    FFT(const FFT &) = delete;
    FFT &operator=(const FFT &) = delete;
    void fftParams(uint32_t fftSize, double /*dBCompensation*/, double sampleRate, int samplesPerBuffer)
    {
        pebblegpu_spectrum_destroy(h);
        h = nullptr;
        status = report("spectrum_create", pebblegpu_spectrum_create(device, fftSize, sampleRate, (uint32_t)samplesPerBuffer, &h));
        bins = 0;
        if (h) pebblegpu_spectrum_bins(h, &bins);
    }
    // the reference's five-argument form (fft.h:29-30, the call SignalSpectrum::setSampleRate makes, signalspectrum.cpp:58-59): the device
    // transform windows with Blackman-Harris only -- any other type leaves no handle and lastStatus() = PEBBLEGPU_E_UNSUPPORTED
    void fftParams(uint32_t fftSize, double dBCompensation, double sampleRate, int samplesPerBuffer, WindowFunction::WINDOWTYPE windowType)
    {
        if (windowType != WindowFunction::BLACKMANHARRIS) {
            pebblegpu_spectrum_destroy(h);
            h = nullptr;
            bins = 0;
            status = PEBBLEGPU_E_UNSUPPORTED;
            std::fprintf(stderr, "pebblegpu: fftParams: window type %d is not implemented on the device (BLACKMANHARRIS only)\n", (int)windowType);
            return;
        }
        fftParams(fftSize, dBCompensation, sampleRate, samplesPerBuffer);
    }
    int getFFTSize() const { return (int)bins; }
    bool fftSpectrum(CPX *in, double *out, int numSamples)
    {
        int ov = 0;
        if (!h) return false;  // "if (!m_fftParamsSet) return false;"
        status = report("spectrum_process", pebblegpu_spectrum_process(h, reinterpret_cast<const double *>(in), numSamples, out, &ov));
        return ov != 0;
    }
    // bool FFT::mapFFTToScreen (fft.h:53-56, fft.cpp:411-534) on the device.  inBuf must be the out of this object's last fftSpectrum
    // call -- what SignalSpectrum always passes (signalspectrum.cpp:146, :164): the library maps its own copy of that spectrum and does
    // not read inBuf.  Returns false, as the reference does; outBuf receives xPixels values (untouched when the call is refused).
    bool mapFFTToScreen(double * /*inBuf*/, int32_t yPixels, int32_t xPixels, double maxdB, double mindB, int32_t startFreq, int32_t stopFreq,
                        int32_t *outBuf)
    {
        if (!h) return false;
        pebblegpu_screen_map m;
        std::memset(&m, 0, sizeof(m));
        m.struct_size = sizeof(m);
        m.y_pixels = yPixels;
        m.x_pixels = xPixels;
        m.max_db = maxdB;
        m.min_db = mindB;
        m.start_freq = startFreq;
        m.stop_freq = stopFreq;
        status = report("spectrum_map_to_screen", pebblegpu_spectrum_map_to_screen(h, &m, outBuf));
        return false;
    }
    int lastStatus() const { return status; }

private:
    pebblegpu_spectrum *h = nullptr;
    uint32_t bins = 0;
    int device, status = 0;
};

// The Morse digital modem (plugins/MorseDigitalModem/morse.h), DigitalModemInterface's processing members.  Where the reference
// appends text, the library hands out the tokens of MorseCode::tokenizeDotDash and word spaces: render them with the application's
// MorseCode::tokenLookup(Morse::dotDash(token)) ("*" when it returns NULL) and " ".
typedef pebblegpu_morse_event MorseEvent;
typedef pebblegpu_morse_report MorseReport;
class Morse {
public:
    explicit Morse(int device = 0) : dev(device) {}
    ~Morse() { pebblegpu_morse_destroy(h); }
    Morse(const Morse &) = delete;
    Morse &operator=(const Morse &) = delete;
    void setSampleRate(int sampleRate, int sampleCount)  // morse.cpp:160-246: a fresh decoder in dmCWL from the current WPM estimate
    {
        if (h) status = report("morse_set_sample_rate", pebblegpu_morse_set_sample_rate(h, (uint32_t)sampleRate, (uint32_t)sampleCount));
        else status = report("morse_create", pebblegpu_morse_create(dev, (uint32_t)sampleRate, (uint32_t)sampleCount, &h));
    }
    void setDemodMode(DemodMode m) { if (h) status = report("morse_set_demod_mode", pebblegpu_morse_set_demod_mode(h, (int)m)); }
    CPX *processBlock(CPX *in)  // morse.cpp:761-894: returns in unchanged
    {
        if (h) status = report("morse_process", pebblegpu_morse_process(h, reinterpret_cast<const double *>(in)));
        return in;
    }
    // the events since the last call, oldest first
    std::vector<MorseEvent> events()
    {
        std::vector<MorseEvent> out;
        MorseEvent buf[256];
        uint32_t got = 256;
        while (h && got == 256) {
            if ((status = report("morse_events", pebblegpu_morse_events(h, buf, 256, &got))) != 0) break;
            out.insert(out.end(), buf, buf + got);
        }
        return out;
    }
    MorseReport getStatus() { MorseReport r{}; if (h) status = report("morse_status", pebblegpu_morse_status(h, &r)); return r; }  // refreshOutput
    // the dot-dash string of a token (the inverse of MorseCode::tokenizeDotDash, morsecode.cpp:160-185), as tokenLookup takes it
    static std::string dotDash(uint32_t token)
    {
        std::string s;
        int top = 31;
        while (top > 0 && !((token >> top) & 1u)) top--;
        for (int b = top - 1; b >= 0; b--) s += ((token >> b) & 1u) ? '-' : '.';
        return s;
    }
    int lastStatus() const { return status; }

private:
    pebblegpu_morse *h = nullptr;
    int dev = 0, status = 0;
};

// The members of TestBench that Receiver::processIQData calls (application/receiver.cpp:797-798; testbench.cpp:518-544) over the
// library's generator, with NCO::initSweep's signature (pebblelib/nco.h:52-55) for the set-up the reference's dialog does.  The two
// calls stay separate, as in the reference: one generator object each, so the sweep's phase and the noise counter advance with their own
// calls.  Results are float-rounded (the library's kernels work on float2).
class TestBench {
public:
    enum SweepType { SINGLE, REPEAT, REPEAT_REVERSE };  // NCO::SweepType, nco.h:52
    TestBench(uint32_t sampleRate, uint32_t bufferSize, int device = 0)
    {
        status = report("siggen_create", pebblegpu_siggen_create(device, (double)sampleRate, bufferSize, &sweepGen));
        if (status == 0) status = report("siggen_create", pebblegpu_siggen_create(device, (double)sampleRate, bufferSize, &noiseGen));
        std::memset(&sw, 0, sizeof(sw));
        sw.struct_size = sizeof(sw);
        sw.amplitude = 1.0;
        sw.mix = 1;
    }
    ~TestBench()
    {
        pebblegpu_siggen_destroy(sweepGen);
        pebblegpu_siggen_destroy(noiseGen);
    }
    TestBench(const TestBench &) = delete;
    TestBench &operator=(const TestBench &) = delete;
    // NCO::initSweep (nco.cpp:119-137) as TestBench::reset calls it (testbench.cpp:557-558): restarts the sweep
    void initSweep(double sweepStartFreq, double sweepStopFreq, double sweepRate, double pulseWidth, double pulsePeriod, SweepType sweepType = SINGLE)
    {
        sw.start_hz = sweepStartFreq;
        sw.stop_hz = sweepStopFreq;
        sw.rate_hz_per_s = sweepRate;
        sw.pulse_width_s = pulseWidth;
        sw.pulse_period_s = pulsePeriod;
        sw.sweep_type = (int32_t)sweepType;
        sweepOn = true;
        apply();
    }
    void setSignalAmplitude(double a) { sw.amplitude = a; if (sweepOn) apply(); }  // m_signalAmplitude (linear), testbench.cpp:563
    void setMix(bool mix) { sw.mix = mix ? 1 : 0; if (sweepOn) apply(); }          // genMixBox, testbench.cpp:521
    void setSweepOn(bool on) { sweepOn = on; if (sweepGen) status = report("siggen_set_sweep", pebblegpu_siggen_set_sweep(sweepGen, on ? &sw : nullptr)); }
    // m_noiseOn + m_noiseAmplitude (linear, testbench.cpp:566); amplitude <= 0: off
    void setNoise(double amplitude, uint64_t seed = 0) { if (noiseGen) status = report("siggen_set_noise", pebblegpu_siggen_set_noise(noiseGen, amplitude, seed)); }
    void genSweep(int length, CPX *pBuf)  // testbench.cpp:518-526
    {
        if (sweepGen && sweepOn && length > 0) status = report("siggen_generate", pebblegpu_siggen_generate(sweepGen, reinterpret_cast<double *>(pBuf), (uint32_t)length));
    }
    void genNoise(int length, CPX *pBuf)  // testbench.cpp:537-544
    {
        if (noiseGen && length > 0) status = report("siggen_generate", pebblegpu_siggen_generate(noiseGen, reinterpret_cast<double *>(pBuf), (uint32_t)length));
    }
    int lastStatus() const { return status; }

private:
    void apply() { if (sweepGen) status = report("siggen_set_sweep", pebblegpu_siggen_set_sweep(sweepGen, &sw)); }
    pebblegpu_siggen *sweepGen = nullptr, *noiseGen = nullptr;
    pebblegpu_sweep sw;
    bool sweepOn = false;
    int status = 0;
};

// The reference's Morse sender (plugins/MorseGenDevice/morsegen.h) over the library's generator: one station per object.  setParams has
// the reference's signature (dbAmplitude in dB: m_amplitude = 10^(dB/20), morsegen.cpp:40); the text is handed over as MorseCode tokens
// (the application keeps MorseCode::asciiLookup; 0 stands for ' '); generate() ADDS the next n samples to out -- the reference's
// per-sample loop "out[i] = ... + m_morseGenN->nextOutputSample()" (morsegendevice.cpp:1013-1061) as one call per station.  As with the
// reference, setParams and setTextOut each start the text over.  Results are float-rounded (the library's kernels work on float2).
class MorseGen {
public:
    explicit MorseGen(double sampleRate, int device = 0)
    {
        status = report("siggen_create", pebblegpu_siggen_create(device, sampleRate, 2048, &gen));
        std::memset(&st, 0, sizeof(st));
        st.struct_size = sizeof(st);
    }
    ~MorseGen() { pebblegpu_siggen_destroy(gen); }
    MorseGen(const MorseGen &) = delete;
    MorseGen &operator=(const MorseGen &) = delete;
    void setParams(double frequency, double dbAmplitude, uint32_t wpm, uint32_t msRise)  // morsegen.cpp:33-160
    {
        st.frequency_hz = frequency;
        st.amplitude = std::pow(10.0, dbAmplitude / 20.0);  // DB::dBToAmplitude
        st.wpm = wpm;
        st.ms_rise = msRise;
        apply();
    }
    void setTextOut(const std::vector<uint16_t> &tokensOut)  // morsegen.cpp:163-180
    {
        tokens = tokensOut;
        apply();
    }
    bool hasOutputSamples() const { return !tokens.empty(); }  // the text repeats: always, once there is one
    void generate(CPX *out, uint32_t n)
    {
        if (gen && on && n > 0) status = report("siggen_generate", pebblegpu_siggen_generate(gen, reinterpret_cast<double *>(out), n));
    }
    int lastStatus() const { return status; }

private:
    void apply()
    {
        if (!gen) return;
        on = false;
        if (tokens.empty() || st.wpm == 0) { status = report("siggen_set_morse", pebblegpu_siggen_set_morse(gen, nullptr, 0, 1)); return; }  // nothing to send yet
        st.tokens = tokens.data();
        st.n_tokens = (uint32_t)tokens.size();
        status = report("siggen_set_morse", pebblegpu_siggen_set_morse(gen, &st, 1, 1));
        on = status == 0;
    }
    pebblegpu_siggen *gen = nullptr;
    pebblegpu_morse_station st;
    std::vector<uint16_t> tokens;
    bool on = false;
    int status = 0;
};

// The slice of application/receiver.cpp this library replaces: turnPowerOn's step construction and
// processIQData's DSP for one tuned channel, audio delivered through the CB_ProcessAudioData-shaped callback.
class Receiver {
public:
    // audioOutRate: Key_AudioOutputSampleRate (receiver.cpp:203); 0 keeps the audio at the demod rate
    Receiver(uint32_t sampleRate, uint16_t framesPerBuffer, bool wfm, uint32_t spectrumBins, CB_ProcessAudioData audioCb,
             uint32_t fastfirFft = 0, uint32_t fastfirTaps = 0, int device = 0, uint32_t audioOutRate = 0)
        : n(framesPerBuffer), cb(audioCb), dev(device)
    {
        pebblegpu_config cfg;
        std::memset(&cfg, 0, sizeof(cfg));
        cfg.struct_size = sizeof(cfg);
        cfg.device = device;
        cfg.sample_rate = sampleRate;
        cfg.frames_per_buffer = framesPerBuffer;
        cfg.n_channels = 1;
        cfg.shared_input = 1;
        cfg.wfm = wfm ? 1 : 0;
        cfg.spectrum_bins = spectrumBins;
        cfg.fastfir_fft = fastfirFft;
        cfg.fastfir_taps = fastfirTaps;
        cfg.max_superframes = 1;
        cfg.audio_rate = audioOutRate;
        status = report("receiver_create", pebblegpu_receiver_create(&cfg, &h));
        pebblegpu_info info;
        if (h && pebblegpu_receiver_info(h, &info) == 0) {
            audio.resize((size_t)(info.superframe / info.total_decimation) + framesPerBuffer);
            spectrum.resize(info.spectrum_bins);
            demodRate = info.demod_rate_int;
            superframe = info.superframe;
        }
    }
    ~Receiver()
    {
        if (dIn) pebblegpu_free(dev, dIn);
        if (dPx) pebblegpu_free(dev, dPx);
        pebblegpu_receiver_destroy(h);
    }
    Receiver(const Receiver &) = delete;
    Receiver &operator=(const Receiver &) = delete;
    void mixerChanged(int f) { if (h) status = report("set_mixer_freq", pebblegpu_set_mixer_freq(h, 0, f)); }               // receiver.cpp:709
    void filterChanged(int lo, int hi) { if (h) status = report("set_bandpass", pebblegpu_set_bandpass(h, 0, lo, hi)); }    // receiver.cpp:658
    void demodModeChanged(DemodMode m) { if (h) status = report("set_demod_mode", pebblegpu_set_demod_mode(h, 0, (int)m)); } // receiver.cpp:640
    // agcModeChanged / agcThresholdChanged -> AGC::setAgcMode(mode, threshold) (agc.cpp:53-82)
    void agcModeChanged(int agcMode, int threshold) { if (h) status = report("set_agc", pebblegpu_set_agc(h, 0, agcMode, threshold)); }
    void squelchChanged(double s) { if (h) status = report("set_squelch", pebblegpu_set_squelch(h, 0, s)); }                // receiver.cpp:704
    // setDigitalModem("Morse") / setDigitalModem(NULL) (receiver.cpp:1085-1115) and the Morse decoder's output
    void setMorse(bool on) { if (h) status = report("set_morse", pebblegpu_set_morse(h, 0, on ? 1 : 0)); }
    std::vector<MorseEvent> morseEvents()
    {
        std::vector<MorseEvent> out;
        MorseEvent buf[256];
        uint32_t got = 256;
        while (h && got == 256) {
            if ((status = report("receiver_morse_events", pebblegpu_receiver_morse_events(h, 0, buf, 256, &got))) != 0) break;
            out.insert(out.end(), buf, buf + got);
        }
        return out;
    }
    MorseReport morseStatus() { MorseReport r{}; if (h) status = report("receiver_morse_status", pebblegpu_receiver_morse_status(h, 0, &r)); return r; }
    // The test bench (receiver.cpp:797-803, 945, 953, 979-980, 992).  The generator and the taps live on the library's batched device
    // path: while one of them is on, processIQData collects a super-frame of frames, runs it as one pebblegpu_receiver_process call and
    // hands every tapped point to displayData frame by frame (numSamples, frame, sample rate, point -- TestBench::displayData's
    // arguments) before the audio callback; the unprocessed spectrum is then the super-frame's last frame's.  A host DigitalModemInterface
    // plugin binds its processBlock to PEBBLEGPU_TAP_MODEM here.
    typedef std::function<void(int, CPX *, double, int)> CB_DisplayData;
    void setTestBenchSweep(const pebblegpu_sweep *s) { if (h) status = report("set_testbench_sweep", pebblegpu_set_testbench_sweep(h, s)); if (status == 0) tbSweep = s != nullptr; }
    void setTestBenchNoise(double amplitude, uint64_t seed) { if (h) status = report("set_testbench_noise", pebblegpu_set_testbench_noise(h, amplitude, seed)); if (status == 0) tbNoise = amplitude > 0; }
    // MorseGen stations summed into the input on the device (pebblegpu_set_testbench_morse): n == 0 switches them off
    void setMorseStations(const pebblegpu_morse_station *stations, uint32_t n, bool mix = true)
    {
        if (h) status = report("set_testbench_morse", pebblegpu_set_testbench_morse(h, stations, n, mix ? 1 : 0));
        if (status == 0) tbMorse = n > 0;
    }
    void setTaps(uint32_t mask, CB_DisplayData displayData)
    {
        if (h) status = report("receiver_set_taps", pebblegpu_receiver_set_taps(h, mask));
        if (status == 0) { tapMask = mask; display = displayData; }
    }
    // bound as the device plugin's CB_ProcessIQData, like receiver.cpp:135-138
    void processIQData(CPX *in, uint16_t numSamples)
    {
        if (!h) return;
        if (tbSweep || tbNoise || tbMorse || tapMask || modemOpen) { processBatched(in, numSamples); return; }
        uint32_t na = 0;
        // (behind setUpdatesPerSec a frame the timer skips leaves `spectrum` as it is: the last computed one, as getUnprocessed() holds it)
        status = report("process_iq", pebblegpu_process_iq_updates(h, reinterpret_cast<const double *>(in), numSamples, reinterpret_cast<double *>(audio.data()), &na,
                                                                  spectrum.empty() ? nullptr : spectrum.data(), &specUpdated));
        if (status == 0 && na > 0 && cb) {
            for (uint32_t off = 0; off < na; off += n) cb(audio.data() + off, (uint16_t)((na - off) < n ? (na - off) : n));  // processAudioData, receiver.cpp:1007
        }
    }
    const std::vector<double> &unprocessedSpectrum() const { return spectrum; }  // SignalSpectrum::getUnprocessed
    // SignalSpectrum::setUpdatesPerSec (signalspectrum.cpp:124-135; bound to SpectrumWidget::updatesPerSecChanged): spectra per second
    // on the stream's sample clock, 0 for none; PEBBLEGPU_SPECTRUM_EVERY_FRAME (the library's default) for one per frame
    void setUpdatesPerSec(int updatesPerSec) { if (h) status = report("set_spectrum_updates", pebblegpu_set_spectrum_updates(h, updatesPerSec)); }
    bool spectrumUpdated() const { return specUpdated != 0; }  // the last processIQData made a spectrum (newFftData would have been emitted)
    // bool SignalSpectrum::mapFFTToScreen(qint32 maxHeight, qint32 maxWidth, double maxdB, double mindB, qint32 startFreq,
    // qint32 stopFreq, qint32 *outBuf), signalspectrum.cpp:137-149: the last frame's unprocessed spectrum mapped on the device
    // (pebblegpu_receiver_map_spectrum), maxWidth values into outBuf.  Returns false, as the reference does.
    bool mapFFTToScreen(int32_t maxHeight, int32_t maxWidth, double maxdB, double mindB, int32_t startFreq, int32_t stopFreq, int32_t *outBuf)
    {
        if (!h || !outBuf || maxWidth <= 0) return false;
        uint64_t frames = 0;
        pebblegpu_receiver_spectrum(h, &frames);
        if ((size_t)maxWidth > pxCap) {
            if (dPx) pebblegpu_free(dev, dPx);
            dPx = nullptr;
            pxCap = 0;
            if ((status = report("malloc", pebblegpu_malloc(dev, sizeof(int32_t) * (size_t)maxWidth, &dPx))) != 0) return false;
            pxCap = (size_t)maxWidth;
        }
        pebblegpu_screen_map m;
        std::memset(&m, 0, sizeof(m));
        m.struct_size = sizeof(m);
        m.y_pixels = maxHeight;
        m.x_pixels = maxWidth;
        m.max_db = maxdB;
        m.min_db = mindB;
        m.start_freq = startFreq;
        m.stop_freq = stopFreq;
        status = report("receiver_map_spectrum", pebblegpu_receiver_map_spectrum(h, &m, frames ? (uint32_t)(frames - 1) : 0u, 1, 1, static_cast<int32_t *>(dPx)));
        if (status == 0) status = report("memcpy_d2h", pebblegpu_memcpy_d2h(dev, outBuf, dPx, sizeof(int32_t) * (size_t)maxWidth));
        return false;
    }
    // The modem hook ring (pebblegpu_receiver_modem_out_*): the frames m_iDigitalModem->processBlock receives (receiver.cpp:979-980), in
    // pinned blocks a plugin's thread reads without a synchronize.  Read-only: what the plugin returns never reaches the chain.  While
    // the ring is open processIQData runs on the library's batched device path (pebblegpu_process_iq is refused beside a ring): it
    // collects a super-frame of frames and queues it as one call.  modemOutNext / modemOutRelease may be called from another thread;
    // feedModemBlock (below) turns a block into the reference's processBlock calls.
    int modemOutOpen(int format = PEBBLEGPU_AUDIO_F32, uint32_t nSlots = 4)
    {
        if (h) status = report("receiver_modem_out_open", pebblegpu_receiver_modem_out_open(h, format, nullptr, 0, nSlots));
        if (h && status == 0) modemOpen = true;
        return status;
    }
    // The same ring at a modem rate (pebblegpu_receiver_modem_out_open_rate): every row already through the reference's own Decimator
    // chain for (maxBw, minRate) -- what Morse::setSampleRate builds (morse.cpp:174-193) and the plugin runs at the head of processBlock --
    // on the device.  minRate 0: the reference's minDecimatedSampleRate.  The blocks report the modem's rate and its samples per
    // super-frame; feedModemBlock then takes the MODEM's frame length (the demodulator frame over the chain's decimation).
    int modemOutOpenRate(int format, uint32_t nSlots, uint32_t maxBw, uint32_t minRate)
    {
        if (h) status = report("receiver_modem_out_open_rate", pebblegpu_receiver_modem_out_open_rate(h, format, nullptr, 0, nSlots, maxBw, minRate));
        if (h && status == 0) modemOpen = true;
        return status;
    }
    int modemOutClose()
    {
        if (h) status = report("receiver_modem_out_close", pebblegpu_receiver_modem_out_close(h));
        if (status == 0) modemOpen = false;
        return status;
    }
    // b->host == nullptr: nothing queued (or, with wait false, not copied yet)
    int modemOutNext(bool wait, pebblegpu_modem_block *b)
    {
        std::memset(b, 0, sizeof(*b));
        b->struct_size = sizeof(*b);
        return h ? report("receiver_modem_out_next", pebblegpu_receiver_modem_out_next(h, wait ? 1 : 0, b)) : PEBBLEGPU_E_INVALID;
    }
    int modemOutRelease(uint64_t callIndex) { return h ? report("receiver_modem_out_release", pebblegpu_receiver_modem_out_release(h, callIndex)) : PEBBLEGPU_E_INVALID; }
    uint64_t modemOutDropped() { uint64_t d = 0; if (h) status = report("receiver_modem_out_dropped", pebblegpu_receiver_modem_out_dropped(h, &d)); return d; }
    uint32_t demodSampleRate() const { return demodRate; }
    int lastStatus() const { return status; }

private:
    void processBatched(CPX *in, uint16_t numSamples)
    {
        if (numSamples != n || !superframe) { status = report("process_iq", PEBBLEGPU_E_SIZE); return; }
        if (!dIn && (status = report("malloc", pebblegpu_malloc(dev, sizeof(float) * 2 * (size_t)superframe, &dIn))) != 0) return;
        staged.resize(2 * (size_t)superframe);
        for (size_t i = 0; i < (size_t)n; i++) {
            staged[2 * (filled + i)] = (float)in[i].real();
            staged[2 * (filled + i) + 1] = (float)in[i].imag();
        }
        filled += n;
        if (filled < superframe) return;
        filled = 0;
        if ((status = report("memcpy_h2d", pebblegpu_memcpy_h2d(dev, dIn, staged.data(), sizeof(float) * staged.size()))) != 0) return;
        if ((status = report("receiver_process", pebblegpu_receiver_process(h, dIn, superframe))) != 0) return;
        if ((status = report("receiver_synchronize", pebblegpu_receiver_synchronize(h))) != 0) return;
        static const int points[5] = {PEBBLEGPU_TAP_RAW_IQ, PEBBLEGPU_TAP_POST_MIXER, PEBBLEGPU_TAP_POST_BP, PEBBLEGPU_TAP_MODEM, PEBBLEGPU_TAP_POST_DEMOD};
        for (int pt : points) {
            uint64_t rows = 0, pitch = 0;
            double rate = 0;
            const void *p = (tapMask >> pt & 1u) ? pebblegpu_receiver_tap(h, pt, &rows, &pitch, &rate) : nullptr;
            if (!p || !display) continue;
            fetch(p, (size_t)rows);
            for (size_t off = 0; off + n <= (size_t)rows; off += n) display((int)n, frames.data() + off, rate, pt);
        }
        if (!spectrum.empty()) {
            uint64_t nfr = 0;
            const void *p = pebblegpu_receiver_spectrum(h, &nfr);
            specUpdated = nfr ? 1u : 0u;
            if (p && nfr) {
                stagedSpec.resize(spectrum.size());
                if ((status = report("memcpy_d2h", pebblegpu_memcpy_d2h(dev, stagedSpec.data(), static_cast<const float *>(p) + (nfr - 1) * spectrum.size(), sizeof(float) * spectrum.size()))) != 0) return;
                for (size_t i = 0; i < spectrum.size(); i++) spectrum[i] = (double)stagedSpec[i];
            }
        }
        uint64_t na = 0;
        const void *pa = pebblegpu_receiver_audio(h, &na, nullptr);
        if (!pa || !na || !cb) return;
        fetch(pa, (size_t)na);
        for (size_t off = 0; off < (size_t)na; off += n) cb(frames.data() + off, (uint16_t)((na - off) < n ? (na - off) : n));  // processAudioData, receiver.cpp:1007
    }
    void fetch(const void *dSrc, size_t count)  // device float2 row -> frames (CPX)
    {
        staged.resize(2 * count > staged.size() ? 2 * count : staged.size());
        frames.resize(count);
        if ((status = report("memcpy_d2h", pebblegpu_memcpy_d2h(dev, staged.data(), dSrc, sizeof(float) * 2 * count))) != 0) { frames.assign(count, CPX(0, 0)); return; }
        for (size_t i = 0; i < count; i++) frames[i] = CPX(staged[2 * i], staged[2 * i + 1]);
    }
    pebblegpu_receiver *h = nullptr;
    uint16_t n;
    bool tbSweep = false, tbNoise = false, tbMorse = false, modemOpen = false;
    uint32_t tapMask = 0;
    CB_DisplayData display;
    uint64_t superframe = 0;
    size_t filled = 0;
    void *dIn = nullptr;
    std::vector<float> staged, stagedSpec;
    std::vector<CPX> frames;
    CB_ProcessAudioData cb;
    std::vector<CPX> audio;
    std::vector<double> spectrum;
    uint32_t specUpdated = 0;
    uint32_t demodRate = 0;
    int status = 0;
    int dev;
    void *dPx = nullptr;  // the mapped pixels on the device (mapFFTToScreen)
    size_t pxCap = 0;
};

// A modem block (pebblegpu_modem_block, from any receiver or shard handle) as the calls the reference would have made: one
// processBlock(CPX *in)-shaped callback per demodulator frame (demodFrames samples: the receiver's frames_per_buffer over its
// decimation, DigitalModemInterface::setSampleRate's second argument) of every PRESENT (block row, super-frame), a channel's frames
// in stream order; absent pairs -- a closed squelch, dmNONE: the reference returned before the hook -- are skipped, not delivered as
// zeros.  Samples arrive as the reference's CPX: the float rows widened, PCM16 rows divided by 32767.  Returns the number of callbacks
// (0 as well for a frame length that does not divide the super-frame).  On a ring opened at a modem rate (modemOutOpenRate) the rows
// are at the modem's rate and demodFrames is the MODEM's frame: the demodulator frame over the chain's total decimation.
typedef std::function<void(uint32_t row, CPX *in, uint32_t numSamples)> CB_ModemProcessBlock;
inline uint64_t feedModemBlock(const pebblegpu_modem_block &b, uint32_t demodFrames, const CB_ModemProcessBlock &processBlock)
{
    if (!b.host || !b.present || !b.n_superframes || !demodFrames || b.samples_per_superframe % demodFrames || !processBlock) return 0;
    std::vector<CPX> frame(demodFrames);
    uint64_t calls = 0;
    for (uint32_t r = 0; r < b.n_channels; r++) {
        const char *row = static_cast<const char *>(b.host) + (size_t)r * b.pitch_bytes;
        for (uint32_t j = 0; j < b.n_superframes; j++) {
            if (!b.present[(size_t)r * b.n_superframes + j]) continue;
            for (uint64_t at = j * b.samples_per_superframe; at < (j + 1) * b.samples_per_superframe; at += demodFrames) {
                for (uint32_t i = 0; i < demodFrames; i++) {
                    if (b.format == PEBBLEGPU_AUDIO_F32) {
                        const float *p = reinterpret_cast<const float *>(row) + 2 * (at + i);
                        frame[i] = CPX(p[0], p[1]);
                    } else {
                        const int16_t *p = reinterpret_cast<const int16_t *>(row) + 2 * (at + i);
                        frame[i] = CPX(p[0] / 32767.0, p[1] / 32767.0);
                    }
                }
                processBlock(r, frame.data(), demodFrames);
                calls++;
            }
        }
    }
    return calls;
}

// A bank whose channels are sharded across devices, driven by this one process and one consumer thread (pebblegpu_multibank_*): the
// shape a Qt host needs to use more than one GPU.  Channels are global; the control slots are routed to
// the shard that owns the channel.  The config's n_channels is the total, its device is ignored.
class MultiBank {
public:
    MultiBank(const pebblegpu_config &config, const std::vector<int> &devices, uint32_t flags = 0)
    {
        std::vector<int32_t> ids(devices.begin(), devices.end());
        pebblegpu_config cfg = config;
        cfg.struct_size = sizeof(cfg);
        status = report("multibank_create", pebblegpu_multibank_create(&cfg, ids.data(), (uint32_t)ids.size(), flags, &h));
    }
    ~MultiBank() { pebblegpu_multibank_destroy(h); }
    MultiBank(const MultiBank &) = delete;
    MultiBank &operator=(const MultiBank &) = delete;
    uint32_t shards() const { uint32_t g = 0; if (h) pebblegpu_multibank_shards(h, &g); return g; }
    // shard g's receiver handle, BORROWED: for every pebblegpu_set_* and pebblegpu_receiver_* read-out with channels local to the shard,
    // never for pebblegpu_receiver_destroy or a process / ingest entry point
    pebblegpu_receiver *shard(uint32_t g, int32_t *device = nullptr, uint32_t *firstChannel = nullptr, uint32_t *nChannels = nullptr)
    {
        pebblegpu_receiver *rx = nullptr;
        if (h) status = report("multibank_shard", pebblegpu_multibank_shard(h, g, &rx, device, firstChannel, nChannels));
        return rx;
    }
    void setMixer(uint32_t channel, double f) { uint32_t c; if (pebblegpu_receiver *rx = at(channel, &c)) status = report("set_mixer_freq", pebblegpu_set_mixer_freq(rx, c, f)); }
    void setBandPass(uint32_t channel, double lo, double hi) { uint32_t c; if (pebblegpu_receiver *rx = at(channel, &c)) status = report("set_bandpass", pebblegpu_set_bandpass(rx, c, lo, hi)); }
    void setDemodMode(uint32_t channel, DemodMode m) { uint32_t c; if (pebblegpu_receiver *rx = at(channel, &c)) status = report("set_demod_mode", pebblegpu_set_demod_mode(rx, c, (int)m)); }
    // dIq[g]: float2 input on shard g's device; queue and return (results after synchronize())
    int process(const std::vector<const void *> &dIq, uint64_t n) { return status = h && dIq.size() == shards() ? report("multibank_process", pebblegpu_multibank_process(h, dIq.data(), n)) : PEBBLEGPU_E_INVALID; }
    int processRaw(int format, int iqOrder, double gain, const std::vector<const void *> &dRaw, uint64_t n)
    {
        return status = h && dRaw.size() == shards() ? report("multibank_process_raw", pebblegpu_multibank_process_raw(h, format, iqOrder, gain, dRaw.data(), n)) : PEBBLEGPU_E_INVALID;
    }
    // the pinned slots: acquire, fill, submit, processIngested, slot ^= 1
    void *ingestAcquire(uint32_t slot, uint64_t bytes) { void *p = nullptr; if (h) status = report("multibank_ingest_acquire", pebblegpu_multibank_ingest_acquire(h, slot, bytes, &p)); return p; }
    int ingestSubmit(uint32_t slot, uint64_t bytes) { return status = h ? report("multibank_ingest_submit", pebblegpu_multibank_ingest_submit(h, slot, bytes)) : PEBBLEGPU_E_INVALID; }
    int processIngested(uint32_t slot, int format, int iqOrder, double gain, uint64_t n)
    {
        return status = h ? report("multibank_process_ingested", pebblegpu_multibank_process_ingested(h, slot, format, iqOrder, gain, n)) : PEBBLEGPU_E_INVALID;
    }
    int synchronize() { return status = h ? report("multibank_synchronize", pebblegpu_multibank_synchronize(h)) : PEBBLEGPU_E_INVALID; }
    int lastStatus() const { return status; }
    pebblegpu_multibank *handle() { return h; }

private:
    pebblegpu_receiver *at(uint32_t channel, uint32_t *local)
    {
        uint32_t g = 0;
        if (!h || (status = report("multibank_locate", pebblegpu_multibank_locate(h, channel, &g, local))) != 0) return nullptr;
        return shard(g);
    }
    pebblegpu_multibank *h = nullptr;
    int status = 0;
};

// Qt-free stand-in for plugins/FileSDRDevice: reads a RIFF/WAVE IQ recording (16-bit PCM stereo, /32767 as
// wavfile.cpp:299-300, or float32 stereo) and pumps framesPerBuffer-sized CPX frames into the callback the host bound
// with initialize().  start() runs the whole file synchronously (the reference paces it in real time through
// ProducerConsumer; pacing is host threading, out of scope -- SURVEY.md 2.1).
class FileSdrFeeder {
public:
    bool initialize(CB_ProcessIQData callback, uint16_t framesPerBuffer_)
    {
        cb = callback;
        framesPerBuffer = framesPerBuffer_;
        return true;
    }
    bool connectDevice(const std::string &fileName)
    {
        f = std::fopen(fileName.c_str(), "rb");
        if (!f) return false;
        unsigned char hdr[12];
        if (std::fread(hdr, 1, 12, f) != 12 || std::memcmp(hdr, "RIFF", 4) || std::memcmp(hdr + 8, "WAVE", 4)) return closeFail();
        bool gotFmt = false;
        for (;;) {  // loop over sub-chunks until "data" (wavfile.cpp:66-140)
            unsigned char ck[8];
            if (std::fread(ck, 1, 8, f) != 8) return closeFail();
            const uint32_t size = ck[4] | (ck[5] << 8) | (ck[6] << 16) | ((uint32_t)ck[7] << 24);
            if (!std::memcmp(ck, "fmt ", 4)) {
                unsigned char fm[16];
                if (size < 16 || std::fread(fm, 1, 16, f) != 16) return closeFail();
                format = fm[0] | (fm[1] << 8);
                channels = fm[2] | (fm[3] << 8);
                sampleRate = fm[4] | (fm[5] << 8) | (fm[6] << 16) | ((uint32_t)fm[7] << 24);
                bits = fm[14] | (fm[15] << 8);
                std::fseek(f, (long)(size - 16 + (size & 1)), SEEK_CUR);
                gotFmt = true;
            } else if (!std::memcmp(ck, "data", 4)) {
                dataStart = std::ftell(f);
                dataBytes = size;
                break;
            } else {
                std::fseek(f, (long)(size + (size & 1)), SEEK_CUR);
            }
        }
        if (!gotFmt || channels != 2 || !((format == 1 && bits == 16) || (format == 3 && bits == 32))) return closeFail();
        return true;
    }
    uint32_t getSampleRate() const { return sampleRate; }
    void setIQGain(double g) { gain = g; }       // Key_IQGain, applied by normalizeIQ (deviceinterfacebase.cpp:532-)
    void setIQSwap(bool s) { swapIQ = s; }       // IQO_QI
    // Cmd_Start: deliver every whole frame of the file once; returns the number of frames delivered
    uint64_t start()
    {
        if (!f || !cb || !framesPerBuffer) return 0;
        std::fseek(f, dataStart, SEEK_SET);
        const size_t bps = (format == 1) ? 4 : 8;
        std::vector<unsigned char> raw(bps * framesPerBuffer);
        std::vector<CPX> frame(framesPerBuffer);
        uint64_t frames = 0, left = dataBytes;
        while (left >= raw.size() && std::fread(raw.data(), 1, raw.size(), f) == raw.size()) {
            left -= raw.size();
            for (uint32_t i = 0; i < framesPerBuffer; i++) {
                double l, r;
                if (format == 1) {
                    const int16_t a = (int16_t)(raw[4 * i] | (raw[4 * i + 1] << 8)), b = (int16_t)(raw[4 * i + 2] | (raw[4 * i + 3] << 8));
                    l = a / 32767.0;  // wavfile.cpp:299-300
                    r = b / 32767.0;
                } else {
                    float a, b;
                    std::memcpy(&a, &raw[8 * i], 4);
                    std::memcpy(&b, &raw[8 * i + 4], 4);
                    l = a;
                    r = b;
                }
                frame[i] = swapIQ ? CPX(r * gain, l * gain) : CPX(l * gain, r * gain);
            }
            cb(frame.data(), framesPerBuffer);  // consumerWorker -> processIQData(bufPtr, m_framesPerBuffer), filesdrdevice.cpp:280
            frames++;
        }
        return frames;
    }
    void disconnectDevice()
    {
        if (f) std::fclose(f);
        f = nullptr;
    }
    ~FileSdrFeeder() { disconnectDevice(); }

private:
    bool closeFail()
    {
        disconnectDevice();
        return false;
    }
    std::FILE *f = nullptr;
    CB_ProcessIQData cb;
    uint16_t framesPerBuffer = 0;
    uint32_t sampleRate = 0, dataBytes = 0;
    int format = 0, channels = 0, bits = 0;
    long dataStart = 0;
    double gain = 1.0;
    bool swapIQ = false;
};

}  // namespace pebblegpu
#endif
