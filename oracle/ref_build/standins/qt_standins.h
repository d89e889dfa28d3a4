/* Stand-ins for the few Qt names the reference's DSP sources use, so that those sources compile unmodified
 * without Qt.  Our own text: nothing here is taken from Qt or from the reference.  Only what the DSP classes
 * touch is defined; everything GUI is an empty type. */
#ifndef PEBBLE_ORACLE_QT_STANDINS_H
#define PEBBLE_ORACLE_QT_STANDINS_H
#include <algorithm>
#include <cassert>
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

class QString {
public:
    QString() {}
    QString(const char *t) : s(t ? t : "") {}
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

class QObject {
public:
    QObject(QObject * = nullptr) {}
    virtual ~QObject() {}
};
/* swallows any value: the device interface passes its arguments and results through it, and no driven class reads one */
class QVariant {
public:
    QVariant() {}
    template <typename T> QVariant(const T &) {}
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
