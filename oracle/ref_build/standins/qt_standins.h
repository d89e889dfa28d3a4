/* Stand-ins for the few Qt names the reference's DSP sources use, so that those sources compile unmodified
 * without Qt.  Our own text: nothing here is taken from Qt or from the reference.  Only what the DSP classes
 * touch is defined; everything GUI is an empty type. */
#ifndef PEBBLE_ORACLE_QT_STANDINS_H
#define PEBBLE_ORACLE_QT_STANDINS_H
#include <algorithm>
#include <cassert>
#include <cstdarg>
#include <cstdio>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

typedef int8_t qint8;
typedef uint8_t quint8;
typedef int16_t qint16;
typedef uint16_t quint16;
typedef int32_t qint32;
typedef uint32_t quint32;
typedef long long qint64;
typedef unsigned long long quint64;
typedef double qreal;

#define Q_UNUSED(x) (void)(x);
#define Q_DECL_EXPORT
#define Q_DECL_IMPORT
#define Q_ASSERT(c) assert(c)
#define Q_OBJECT
#define signals public
#define slots
#define emit
#define Q_DECLARE_INTERFACE(a, b)

/* The order of the comparisons matters for NaN, where every comparison is false: Qt's published qglobal.h words them
 * qMin(a, b) = (a < b) ? a : b, qMax(a, b) = (a < b) ? b : a, qBound(min, v, max) = qMax(min, qMin(max, v)), so that
 * qBound of a NaN is the LOWER bound (SignalStrength::fdEstimate bounds 0 / 0 this way).  Written from that published
 * wording as remembered, not checked against an installed Qt. */
template <typename T> inline const T &qMin(const T &a, const T &b) { return (a < b) ? a : b; }
template <typename T> inline const T &qMax(const T &a, const T &b) { return (a < b) ? b : a; }
template <typename T> inline const T &qBound(const T &lo, const T &v, const T &hi) { return qMax(lo, qMin(hi, v)); }

class QMutex {
public:
    void lock() { m.lock(); }
    void unlock() { m.unlock(); }
private:
    std::recursive_mutex m;
};

/* one byte of a QString: the plugins' texts are Latin-1 (a multi-byte display string of the Morse table is only ever copied whole) */
class QChar {
public:
    QChar() : c(0) {}
    QChar(char v) : c(v) {}
    char toLatin1() const { return c; }
private:
    char c;
};

class QString {
public:
    QString() {}
    QString(const char *t) : s(t ? t : "") {}
    bool isEmpty() const { return s.empty(); }
    int length() const { return int(s.size()); }
    void clear() { s.clear(); }
    QChar at(int i) const { return QChar(s[size_t(i)]); }
    QChar operator[](int i) const { return at(i); }
    QString &append(const QString &o) { s += o.s; return *this; }
    QString toLower() const
    {
        QString r(*this);
        for (char &c : r.s)
            if (c >= 'A' && c <= 'Z')
                c = char(c - 'A' + 'a');
        return r;
    }
    /* replaces every occurrence of the lowest-numbered %N place marker */
    QString arg(const QString &a) const
    {
        int low = 100;
        for (size_t i = 0; i + 1 < s.size(); i++)
            if (s[i] == '%' && s[i + 1] >= '1' && s[i + 1] <= '9')
                low = std::min(low, s[i + 1] - '0');
        QString r;
        for (size_t i = 0; i < s.size(); i++)
            if (i + 1 < s.size() && s[i] == '%' && s[i + 1] - '0' == low) {
                r.s += a.s;
                i++;
            } else
                r.s += s[i];
        return r;
    }
    QString &sprintf(const char *fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        s = buf;
        return *this;
    }
    static QString number(long long v) { return QString(std::to_string(v).c_str()); }
    std::string s;
};

/* null sink: whatever is streamed into it is dropped */
class QDebug {
public:
    template <typename T> QDebug &operator<<(const T &) { return *this; }
    QDebug &noquote() { return *this; }
    QDebug &nospace() { return *this; }
};
inline QDebug qDebug() { return QDebug(); }
inline QDebug qWarning() { return QDebug(); }

struct QIODevice { enum OpenModeFlag { ReadOnly = 1, WriteOnly = 2 }; };
/* never opens: the reference's coefficient dumps are compiled out or skipped */
class QFile {
public:
    QFile() {}
    QFile(const QString &) {}
    void setFileName(const QString &) {}
    bool open(int) { return false; }
    qint64 write(const char *, qint64 n = 0) { return n; }
    void close() {}
};
class QDir {
public:
    static bool setCurrent(const QString &) { return false; }
};

/* connections are never made: whoever wants a signal's effect defines the signal's body (ref_driver.cpp) */
#define SIGNAL(x) #x
#define SLOT(x) #x
#define Q_PLUGIN_METADATA(x)
#define Q_INTERFACES(x)
class QObject {
public:
    QObject(QObject * = nullptr) {}
    virtual ~QObject() {}
    template <typename... A> static bool connect(const A &...) { return false; }
};
/* swallows any value: the device interface passes its arguments and results through it, and no driven class reads one */
class QVariant {
public:
    QVariant() {}
    template <typename T> QVariant(const T &) {}
    int toInt() const { return 0; }
};
class QStringList {};
class QWidget;
class QSize {};
class QMainWindow {};
class QScreen {};
class QSoundEffect {};
class QCoreApplication {};

/* the display-rate gate of the reference's meters is held open: elapsed() is always past any interval */
class QElapsedTimer {
public:
    bool isValid() const { return started; }
    void start() { started = true; }
    qint64 elapsed() const { return started ? (qint64(1) << 40) : 0; }
private:
    bool started = false;
};

template <typename T> class QVector {
public:
    void append(const T &t) { v.push_back(t); }
    int length() const { return int(v.size()); }
    int size() const { return int(v.size()); }
    int count() const { return int(v.size()); }
    bool isEmpty() const { return v.empty(); }
    void clear() { v.clear(); }
    T &operator[](int i) { return v[size_t(i)]; }
    const T &operator[](int i) const { return v[size_t(i)]; }
    const T &at(int i) const { return v[size_t(i)]; }
    T &last() { return v.back(); }
private:
    std::vector<T> v;
};
#endif
