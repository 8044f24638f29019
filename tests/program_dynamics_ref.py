"""The dynamics stage of the programme loudness bank, restated (include/omx/program_dynamics.h holds the definition).

numpy and Python integers only; nothing here calls the library.  `render` is the fast form (whole arrays), `render_slow` evaluates
the definition frame by frame in Python integers, `Stream` is the streaming form that carries state from call to call.
"""
import math

import numpy as np

L_MIN, L_MAX = -40 * 65536, 8 * 65536
MAX_GAIN = 40 * 65536
MAX_STEP = 40 << 32
OCTAVE_DB = 6.020599913279624
BYPASS = 0xFFFFFFFF
POINTS = 769

# LOG[i] = floor(65536 * log2(1 + i / 256))
LOG = [
    0, 368, 735, 1101, 1465, 1828, 2190, 2550, 2909, 3266, 3622, 3977, 4331, 4683, 5034, 5383,
    5731, 6078, 6424, 6769, 7112, 7454, 7794, 8134, 8472, 8809, 9145, 9480, 9813, 10146, 10477, 10807,
    11136, 11463, 11790, 12115, 12440, 12763, 13085, 13406, 13726, 14045, 14363, 14680, 14995, 15310, 15624, 15936,
    16248, 16558, 16868, 17176, 17484, 17790, 18096, 18400, 18704, 19006, 19308, 19608, 19908, 20207, 20505, 20801,
    21097, 21392, 21686, 21980, 22272, 22563, 22854, 23143, 23432, 23720, 24007, 24293, 24578, 24862, 25146, 25429,
    25710, 25991, 26272, 26551, 26829, 27107, 27384, 27660, 27935, 28210, 28483, 28756, 29028, 29300, 29570, 29840,
    30109, 30377, 30644, 30911, 31177, 31442, 31707, 31971, 32234, 32496, 32757, 33018, 33278, 33538, 33796, 34054,
    34312, 34568, 34824, 35079, 35334, 35588, 35841, 36093, 36345, 36596, 36847, 37096, 37346, 37594, 37842, 38089,
    38336, 38582, 38827, 39071, 39315, 39559, 39801, 40044, 40285, 40526, 40766, 41006, 41245, 41483, 41721, 41959,
    42195, 42431, 42667, 42902, 43136, 43370, 43603, 43836, 44068, 44299, 44530, 44760, 44990, 45219, 45448, 45676,
    45904, 46131, 46357, 46583, 46808, 47033, 47257, 47481, 47704, 47927, 48149, 48371, 48592, 48813, 49033, 49253,
    49472, 49690, 49909, 50126, 50343, 50560, 50776, 50992, 51207, 51421, 51635, 51849, 52062, 52275, 52487, 52699,
    52910, 53121, 53331, 53541, 53751, 53960, 54168, 54376, 54584, 54791, 54998, 55204, 55410, 55615, 55820, 56024,
    56228, 56432, 56635, 56837, 57040, 57242, 57443, 57644, 57844, 58044, 58244, 58443, 58642, 58841, 59039, 59236,
    59433, 59630, 59827, 60023, 60218, 60413, 60608, 60802, 60996, 61190, 61383, 61576, 61768, 61960, 62152, 62343,
    62534, 62724, 62914, 63104, 63293, 63482, 63671, 63859, 64047, 64234, 64421, 64608, 64794, 64980, 65165, 65351,
    65536]

# EXP[i] = floor(2^(40 + i / 256))
EXP = [
    1099511627776, 1102492706219, 1105481867187, 1108479132592, 1111484524408, 1114498064667, 1117519775463, 1120549678949,
    1123587797336, 1126634152897, 1129688767967, 1132751664938, 1135822866265, 1138902394464, 1141990272111, 1145086521843,
    1148191166360, 1151304228422, 1154425730852, 1157555696533, 1160694148413, 1163841109498, 1166996602861, 1170160651634,
    1173333279013, 1176514508258, 1179704362691, 1182902865696, 1186110040722, 1189325911283, 1192550500952, 1195783833372,
    1199025932245, 1202276821339, 1205536524488, 1208805065589, 1212082468604, 1215368757560, 1218663956549, 1221968089729,
    1225281181323, 1228603255620, 1231934336973, 1235274449804, 1238623618600, 1241981867914, 1245349222365, 1248725706641,
    1252111345494, 1255506163745, 1258910186282, 1262323438060, 1265745944103, 1269177729501, 1272618819414, 1276069239067,
    1279529013757, 1282998168848, 1286476729773, 1289964722033, 1293462171200, 1296969102913, 1300485542882, 1304011516888,
    1307547050779, 1311092170475, 1314646901965, 1318211271310, 1321785304641, 1325369028159, 1328962468137, 1332565650920,
    1336178602922, 1339801350631, 1343433920605, 1347076339476, 1350728633945, 1354390830790, 1358062956858, 1361745039070,
    1365437104419, 1369139179973, 1372851292872, 1376573470330, 1380305739634, 1384048128148, 1387800663306, 1391563372619,
    1395336283672, 1399119424125, 1402912821712, 1406716504243, 1410530499603, 1414354835754, 1418189540733, 1422034642651,
    1425890169698, 1429756150140, 1433632612317, 1437519584650, 1441417095634, 1445325173843, 1449243847926, 1453173146612,
    1457113098708, 1461063733098, 1465025078745, 1468997164689, 1472980020050, 1476973674028, 1480978155900, 1484993495024,
    1489019720837, 1493056862855, 1497104950676, 1501164013976, 1505234082514, 1509315186126, 1513407354733, 1517510618335,
    1521625007013, 1525750550930, 1529887280332, 1534035225544, 1538194416978, 1542364885123, 1546546660554, 1550739773929,
    1554944255987, 1559160137553, 1563387449533, 1567626222919, 1571876488785, 1576138278291, 1580411622681, 1584696553282,
    1588993101509, 1593301298861, 1597621176920, 1601952767356, 1606296101926, 1610651212470, 1615018130917, 1619396889281,
    1623787519664, 1628190054252, 1632604525324, 1637030965240, 1641469406452, 1645919881500, 1650382423009, 1654857063696,
    1659343836364, 1663842773908, 1668353909308, 1672877275637, 1677412906057, 1681960833818, 1686521092262, 1691093714821,
    1695678735018, 1700276186465, 1704886102868, 1709508518022, 1714143465815, 1718790980226, 1723451095327, 1728123845282,
    1732809264348, 1737507386873, 1742218247301, 1746941880167, 1751678320100, 1756427601826, 1761189760160, 1765964830015,
    1770752846399, 1775553844411, 1780367859250, 1785194926207, 1790035080670, 1794888358123, 1799754794146, 1804634424416,
    1809527284706, 1814433410886, 1819352838923, 1824285604882, 1829231744927, 1834191295318, 1839164292415, 1844150772674,
    1849150772653, 1854164329007, 1859191478491, 1864232257960, 1869286704369, 1874354854772, 1879436746325, 1884532416284,
    1889641902005, 1894765240948, 1899902470672, 1905053628838, 1910218753212, 1915397881658, 1920591052145, 1925798302747,
    1931019671637, 1936255197094, 1941504917501, 1946768871343, 1952047097213, 1957339633804, 1962646519918, 1967967794460,
    1973303496441, 1978653664977, 1984018339292, 1989397558714, 1994791362680, 2000199790732, 2005622882520, 2011060677802,
    2016513216442, 2021980538414, 2027462683800, 2032959692790, 2038471605683, 2043998462888, 2049540304923, 2055097172416,
    2060669106105, 2066256146839, 2071858335578, 2077475713390, 2083108321459, 2088756201078, 2094419393652, 2100097940699,
    2105791883849, 2111501264844, 2117226125542, 2122966507912, 2128722454037, 2134494006116, 2140281206459, 2146084097495,
    2151902721764, 2157737121924, 2163587340747, 2169453421123, 2175335406057, 2181233338669, 2187147262199, 2193077220002,
    2199023255552]

_LOG = np.array(LOG, np.int64)
_EXP = np.array(EXP, np.int64)


class Curve:
    """omx_program_dynamics_curve: T[769] and the detector mask, attack, hold and release step."""

    def __init__(self, T, detector_mask=0xFF, attack=1, hold=0, step=MAX_STEP):
        self.T = np.asarray(T, np.int64).copy()
        assert self.T.shape == (POINTS,)
        self.mask, self.A, self.H, self.d = int(detector_mask), int(attack), int(hold), int(step)

    @property
    def latency(self):
        return self.A - 1


# ---- design (the header's DESIGN FORMULAS)
def entry(g_db):
    lim = 40.0 * OCTAVE_DB
    g = min(max(g_db, -lim), lim)
    return int(math.floor(g / OCTAVE_DB * 65536.0 + 0.5))


def entry_level_db(k):
    return float(L_MIN + 4096 * k) / 65536.0 * OCTAVE_DB


def design(threshold_db, ratio, knee_db=0.0, expander_threshold_db=0.0, expander_ratio=1.0, range_db=math.inf, makeup_db=0.0):
    slope = 1.0 / ratio - 1.0
    T = []
    for k in range(POINTS):
        x = entry_level_db(k)
        c = x - threshold_db
        if 2.0 * c < -knee_db:
            gc = 0.0
        elif knee_db > 0.0 and abs(2.0 * c) <= knee_db:
            gc = slope * ((c + knee_db / 2.0) * (c + knee_db / 2.0)) / (2.0 * knee_db)
        else:
            gc = slope * c
        ge = 0.0
        if expander_ratio != 1.0 and x < expander_threshold_db:
            ge = max((x - expander_threshold_db) * (expander_ratio - 1.0), -range_db)
        T.append(entry(gc + ge + makeup_db))
    return np.array(T, np.int64)


def from_points(points):
    p = [(float(a), float(b)) for a, b in points]
    T = []
    for k in range(POINTS):
        x = entry_level_db(k)
        if x <= p[0][0]:
            g = p[0][1] - p[0][0]
        elif x >= p[-1][0]:
            g = p[-1][1] - p[-1][0]
        else:
            q = 0
            while x >= p[q + 1][0]:
                q += 1
            y = p[q][1] + (x - p[q][0]) * ((p[q + 1][1] - p[q][1]) / (p[q + 1][0] - p[q][0]))
            g = y - x
        T.append(entry(g))
    return np.array(T, np.int64)


def curve_at(T, L):
    """Gt of levels L (array or int): the header's Curve"""
    u = np.asarray(L, np.int64) - L_MIN
    k, f = u >> 12, u & 4095
    T = np.asarray(T, np.int64)
    lo = T[k]
    hi = T[np.minimum(k + 1, POINTS - 1)]
    return np.where(f == 0, lo, lo + (((hi - lo) * f + 2048) >> 12))


def gain_db(T, level_db):
    v = level_db / OCTAVE_DB * 65536.0 + 0.5
    L = L_MIN if v <= L_MIN else (L_MAX if v >= L_MAX + 1 else int(math.floor(v)))
    return float(int(curve_at(T, L))) * (OCTAVE_DB / 65536.0)


def time(fs, attack_ms, hold_ms, release_db_per_s):
    a = max(1.0, math.floor(attack_ms * fs / 1000.0 + 0.5))
    h = math.floor(hold_ms * fs / 1000.0 + 0.5)
    d = math.inf if math.isinf(release_db_per_s) else math.floor(release_db_per_s / OCTAVE_DB * 4294967296.0 / fs + 0.5)
    return int(a), int(h), MAX_STEP if d >= MAX_STEP else (1 if d < 1.0 else int(d))


def emitted(latency, n, e, flush):
    return n if flush else max(e, n - latency if n > latency else 0)


# ---- the signal path
def level(key, mask):
    """L[n] of key f32 [N][C] under a detector mask"""
    key = np.asarray(key, np.float32)
    chans = [c for c in range(key.shape[1]) if (mask >> c) & 1]
    a = np.zeros(key.shape[0], np.float32)
    for c in chans:
        a = np.fmax(a, np.abs(key[:, c]))  # fmax ignores a NaN; a frame of NaN stays 0
    bits = a.view(np.uint32).astype(np.int64)
    e = (bits >> 23) - 127
    m = bits & 0x7FFFFF
    i, f = m >> 15, m & 0x7FFF
    L = e * 65536 + _LOG[i] + (((_LOG[np.minimum(i + 1, 256)] - _LOG[i]) * f + (1 << 14)) >> 15)
    with np.errstate(invalid="ignore"):
        L = np.where(~(a >= np.float32(2.0 ** -40)), L_MIN, np.where(a >= np.float32(256.0), L_MAX, L))
    return L.astype(np.int64)


def target(curve, key):
    return curve_at(curve.T, level(key, curve.mask))


def sliding_min(g, W):
    """w[n] = min(g[n-W+1 .. n]) for the n of g whose whole window lies in g: len(g) - W + 1 values, by doubling"""
    b = np.array(g, np.int64)
    win = 1
    while 2 * win <= W:
        b[win:] = np.minimum(b[win:], b[:-win].copy())
        win *= 2
    # b[k] = min of the `win` values that end at k, win <= W < 2 win
    return np.minimum(b[W - 1:], b[win - 1:len(b) - (W - win)])


def factor(E):
    E = np.asarray(E, np.int64)
    I, F = E >> 32, E & 0xFFFFFFFF
    i, g = F >> 24, F & 0xFFFFFF
    fx = _EXP[i] + (((_EXP[i + 1] - _EXP[i]) * g) >> 24)
    return np.ldexp(fx.astype(np.float64), (I - 40).astype(np.int32))


def apply(x, E):
    """out f32 [n][C] of the frames x under the gains E"""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(all="ignore"):
        y = (x.astype(np.float64) * factor(E)[:, None]).astype(np.float32)
    unity = np.asarray(E) == 0
    y[unity] = x[unity]  # the bits, NaN payloads and -0.0f included
    return y


def trace(E):
    return (np.asarray(E, np.int64).astype(np.float64) * (OCTAVE_DB / 4294967296.0)).astype(np.float32)


def envelope(curve, Gt, flushed=True):
    """(r, E) of a whole stream's Gt: r[n] for n = 0 .. N + LA - 1 and E[j] for every frame (flushed), or the frames a stream that is
    not flushed has emitted.  The fast form: whole arrays."""
    A, W, d, t0 = curve.A, curve.A + curve.H, curve.d, int(curve.T[0])
    Gt = np.asarray(Gt, np.int64)
    N = len(Gt)
    ext = np.concatenate([np.full(W - 1, t0, np.int64), Gt, np.full(A - 1 if flushed else 0, t0, np.int64)])
    w = sliding_min(ext, W) << 16                        # n = 0 .. N + LA - 1
    n = np.arange(len(w), dtype=object)
    v = np.array([int(a) for a in w], dtype=object) - n * d
    run = np.minimum.accumulate(np.concatenate([[t0 * 65536 + d], v]))[1:]   # (r[-1] = T[0] 2^16 sits at index -1: minus (-1) d)
    r = (run + n * d).astype(np.int64) if len(w) else np.zeros(0, np.int64)
    cs = np.concatenate([np.zeros(1, np.int64), np.cumsum(r)])
    n_out = N if flushed else max(N - (A - 1), 0)
    S = cs[A:A + n_out] - cs[:n_out]                     # sum r[j .. j + A - 1]
    return r, S // A


def render(curve, x, key=None, flushed=True):
    """(out f32 [n][C], gain trace f32 [n], E) of a whole stream"""
    x = np.ascontiguousarray(x, np.float32)
    Gt = target(curve, x if key is None else key)
    _r, E = envelope(curve, Gt, flushed)
    return apply(x[:len(E)], E), trace(E), E


def render_slow(curve, x, key=None):
    """E of a whole flushed stream, frame by frame in Python integers: O(N W)"""
    A, W, d, t0 = curve.A, curve.A + curve.H, curve.d, int(curve.T[0])
    Gt = [int(v) for v in target(curve, x if key is None else key)]
    N = len(Gt)

    def gt(n):
        return Gt[n] if 0 <= n < N else t0

    r, prev = {}, t0 << 16
    for n in range(-A - 1, N + A):
        if n < -A:
            r[n] = prev
            continue
        w = min(gt(m) for m in range(n - W + 1, n + 1))
        prev = min(w << 16, prev + d)
        r[n] = prev
    return np.array([sum(r[n] for n in range(j, j + A)) // A for j in range(N)], np.int64), Gt


class Stream:
    """One stream of the stage, call by call: carries the newest Gt, r and PCM as the bank's rings do."""

    def __init__(self, curve, channels):
        self.c, self.C = curve, channels
        t0 = int(curve.T[0])
        self.n = self.e = 0
        self.flushed = False
        self.gt = [t0] * (curve.A + curve.H - 1)          # the newest W - 1 values
        self.r = []                                       # r of the frames taken and not yet emitted past
        self.r_last = t0 << 16
        self.x = np.zeros((0, channels), np.float32)      # frames taken and not emitted
        self.E_all = []

    def push(self, x, key=None, flush=False):
        c = self.c
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.C)
        assert not (self.flushed and len(x))
        k = x if key is None else np.ascontiguousarray(key, np.float32).reshape(-1, self.C)
        Gt = [int(v) for v in target(c, k)]
        if flush and not self.flushed:
            Gt = Gt + [int(c.T[0])] * c.latency
        W = c.A + c.H
        for g in Gt:
            self.gt.append(g)
            self.gt = self.gt[-W:]
            self.r_last = min(min(self.gt) << 16, self.r_last + c.d)
            self.r.append(self.r_last)
        self.x = np.concatenate([self.x, x])
        self.n += len(x)
        self.flushed = self.flushed or flush
        e_new = emitted(c.latency, self.n, self.e, self.flushed)
        k = e_new - self.e
        E = np.array([sum(self.r[j:j + c.A]) // c.A for j in range(k)], np.int64)
        out = apply(self.x[:k], E)
        self.x, self.r = self.x[k:], self.r[k:]
        self.e = e_new
        self.E_all.extend(int(v) for v in E)
        return out, trace(E), E


def record(E, out):
    """the integer fields of omx_program_dynamics_record of everything a stream has emitted"""
    E = np.asarray(E, np.int64)
    out = np.asarray(out, np.float32)
    mag = np.abs(out)
    with np.errstate(invalid="ignore"):
        over = int(np.count_nonzero(mag > np.float32(1.0)))
    peak = float(np.fmax.reduce(mag.reshape(-1), initial=np.float32(0.0))) if out.size else 0.0
    return dict(frames_reduced=int(np.count_nonzero(E < 0)), frames_boosted=int(np.count_nonzero(E > 0)),
                min_gain=int(min(0, E.min())) if E.size else 0, max_gain=int(max(0, E.max())) if E.size else 0,
                samples_over=over, samples_nonfinite=int(np.count_nonzero(~np.isfinite(out))), out_sample_peak=np.float32(peak))
