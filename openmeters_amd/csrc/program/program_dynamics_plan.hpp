// The host-only half of the programme bank's dynamics stage (include/omx/program_dynamics.h): the tables of constants, plan, check,
// latency, design, points, gain, time and the streaming formula.  Plain C++ doubles and integers, no device and no HIP:
// program_dynamics.cpp wraps these for the C ABI, tools/dynamics_design_check.cpp drives them under the sanitizers.  Every function
// returns an OMX_* code and, refusing, the reason in *why; a refusal writes nothing.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../../include/omx/program_dynamics.h"
#include "program_carried.hpp"

namespace omx {

constexpr uint32_t kDyThreads = 256;            // threads per workgroup of every pass
constexpr uint32_t kDyLevelTile = 2048;         // frames per workgroup of the level pass
constexpr uint32_t kDyHoldTile = 2048;          // values per workgroup of the hold pass
constexpr uint32_t kDyHoldMaxWindow = 2048;     // longest window one hold tile takes in LDS
constexpr uint32_t kDyReleasePer = 8;           // consecutive values a thread of the release scan keeps in registers
constexpr uint32_t kDyReleaseTile = kDyThreads * kDyReleasePer;  // values per workgroup of the release scan: one carry each
constexpr uint32_t kDySmoothTile = 1024;        // frames per workgroup of the smooth-and-apply pass
constexpr int32_t kDyLMin = OMX_DYNAMICS_L_MIN, kDyLMax = OMX_DYNAMICS_L_MAX;
constexpr int64_t kDyCap = OMX_DYNAMICS_MAX_STEP;  // 40 * 2^32: no r exceeds it, the ramp term saturates here
constexpr double kDyOctave = OMX_DYNAMICS_OCTAVE_DB;

// LOG[i] = floor(65536 * log2(1 + i / 256))
constexpr int32_t kDyLog[257] = {
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
    65536};

// EXP[i] = floor(2^(40 + i / 256))
constexpr uint64_t kDyExp[257] = {
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
    2199023255552};

inline int dy_fail(const char** why, const char* text) {
    if (why) *why = text;
    return OMX_ERR_INVALID;
}

inline int dy_plan(uint32_t channels, omx_program_dynamics_info* info, const char** why) {
    if (!info) return dy_fail(why, "null info");
    if (channels < 1 || channels > OMX_MAX_CHANNELS) return dy_fail(why, "channels outside 1 .. 8");
    *info = omx_program_dynamics_info{kDyLevelTile, kDyHoldTile, kDyHoldMaxWindow, kDyReleaseTile, kDySmoothTile, kDyThreads, channels, 0u};
    return OMX_NONE;
}

inline bool dy_table_ok(const int32_t* T) {
    for (uint32_t k = 0; k < OMX_DYNAMICS_CURVE_POINTS; ++k)
        if (T[k] > OMX_DYNAMICS_MAX_GAIN || T[k] < -OMX_DYNAMICS_MAX_GAIN) return false;
    return true;
}

inline int dy_check(const omx_program_dynamics_curve* c, const char** why) {
    if (!c) return dy_fail(why, "null curve");
    if (!dy_table_ok(c->T)) return dy_fail(why, "a table entry beyond OMX_DYNAMICS_MAX_GAIN");
    if (c->detector_mask == 0 || c->detector_mask >= (1u << OMX_MAX_CHANNELS))
        return dy_fail(why, "detector_mask 0 or with a bit at or above bit 8");
    if (c->attack_frames < 1 || c->attack_frames > OMX_DYNAMICS_MAX_ATTACK) return dy_fail(why, "attack_frames outside 1 .. 4096");
    if (c->hold_frames > OMX_DYNAMICS_MAX_HOLD) return dy_fail(why, "hold_frames above 16384");
    if (c->release_step < 1 || c->release_step > OMX_DYNAMICS_MAX_STEP) return dy_fail(why, "release_step outside 1 .. OMX_DYNAMICS_MAX_STEP");
    return OMX_NONE;
}

inline int dy_latency(const omx_program_dynamics_curve* c, uint32_t* frames, const char** why) {
    if (!frames) return dy_fail(why, "null frames");
    const int rc = dy_check(c, why);
    if (rc != OMX_NONE) return rc;
    *frames = c->attack_frames - 1;
    return OMX_NONE;
}

inline int dy_frames(uint32_t latency, uint64_t n_before, uint64_t e_before, uint64_t frames, uint32_t flush, uint64_t* frames_out,
                     const char** why) {
    if (!frames_out) return dy_fail(why, "null frames_out");
    if (latency > OMX_DYNAMICS_MAX_ATTACK - 1) return dy_fail(why, "latency above 4095");
    if (n_before > (1ull << 63) || frames > (1ull << 63) - n_before) return dy_fail(why, "frames_in_before + frames beyond 2^63");
    if (e_before > n_before) return dy_fail(why, "frames_out_before above frames_in_before");
    *frames_out = carry_emitted(latency, n_before + frames, e_before, flush != 0) - e_before;
    return OMX_NONE;
}

// the table's gain at a level: the header's Curve (the kernel runs the same integer steps)
inline int32_t dy_curve_at(const int32_t* T, int32_t L) {
    const uint32_t u = (uint32_t)(L - kDyLMin), k = u >> 12, f = u & 4095u;
    if (f == 0) return T[k];
    return T[k] + (int32_t)((((int64_t)T[k + 1] - (int64_t)T[k]) * (int64_t)f + 2048) >> 12);
}

inline int32_t dy_entry(double g_db) {  // a gain in dB as a table entry
    const double lim = 40.0 * kDyOctave;
    const double g = std::min(std::max(g_db, -lim), lim);
    return (int32_t)std::floor(g / kDyOctave * 65536.0 + 0.5);
}
inline double dy_entry_level_db(uint32_t k) { return (double)(kDyLMin + 4096 * (int32_t)k) / 65536.0 * kDyOctave; }

inline int dy_design(const omx_program_dynamics_spec* s, omx_program_dynamics_curve* curve, const char** why) {
    if (!s || !curve) return dy_fail(why, "null pointer");
    const auto level_ok = [](double v) { return std::isfinite(v) && v >= -240.0 && v <= 48.0; };
    if (!level_ok(s->threshold_db)) return dy_fail(why, "threshold_db not finite or outside [-240, 48]");
    if (!(s->ratio >= 1.0)) return dy_fail(why, "ratio below 1 or NaN");
    if (!std::isfinite(s->knee_db) || s->knee_db < 0.0) return dy_fail(why, "knee_db negative or not finite");
    if (!std::isfinite(s->expander_ratio) || s->expander_ratio < 1.0) return dy_fail(why, "expander_ratio below 1 or not finite");
    if (s->expander_ratio != 1.0 && !level_ok(s->expander_threshold_db))
        return dy_fail(why, "expander_threshold_db not finite or outside [-240, 48]");
    if (!(s->range_db >= 0.0)) return dy_fail(why, "range_db negative or NaN");
    if (!std::isfinite(s->makeup_db)) return dy_fail(why, "makeup_db not finite");
    const double slope = 1.0 / s->ratio - 1.0, knee = s->knee_db;
    for (uint32_t k = 0; k < OMX_DYNAMICS_CURVE_POINTS; ++k) {
        const double x = dy_entry_level_db(k), c = x - s->threshold_db;
        double gc;
        if (2.0 * c < -knee) gc = 0.0;
        else if (knee > 0.0 && std::fabs(2.0 * c) <= knee) gc = slope * ((c + knee / 2.0) * (c + knee / 2.0)) / (2.0 * knee);
        else gc = slope * c;
        double ge = 0.0;
        if (s->expander_ratio != 1.0 && x < s->expander_threshold_db)
            ge = std::max((x - s->expander_threshold_db) * (s->expander_ratio - 1.0), -s->range_db);
        curve->T[k] = dy_entry(gc + ge + s->makeup_db);
    }
    return OMX_NONE;
}

inline int dy_from_points(const omx_program_dynamics_point* p, uint32_t n, omx_program_dynamics_curve* curve, const char** why) {
    if (!p || !curve) return dy_fail(why, "null pointer");
    if (n < 1 || n > OMX_DYNAMICS_MAX_POINTS) return dy_fail(why, "n 0 or above OMX_DYNAMICS_MAX_POINTS");
    for (uint32_t i = 0; i < n; ++i) {
        if (!std::isfinite(p[i].in_db) || !std::isfinite(p[i].out_db)) return dy_fail(why, "a value that is not finite");
        if (i != 0 && !(p[i].in_db > p[i - 1].in_db)) return dy_fail(why, "in_db not strictly increasing");
    }
    for (uint32_t k = 0; k < OMX_DYNAMICS_CURVE_POINTS; ++k) {
        const double x = dy_entry_level_db(k);
        double g;
        if (x <= p[0].in_db) g = p[0].out_db - p[0].in_db;
        else if (x >= p[n - 1].in_db) g = p[n - 1].out_db - p[n - 1].in_db;
        else {
            uint32_t q = 0;
            while (x >= p[q + 1].in_db) ++q;  // (x < the last in_db: q + 1 stays below n)
            const double y = p[q].out_db + (x - p[q].in_db) * ((p[q + 1].out_db - p[q].out_db) / (p[q + 1].in_db - p[q].in_db));
            g = y - x;
        }
        curve->T[k] = dy_entry(g);
    }
    return OMX_NONE;
}

inline int dy_gain_db(const omx_program_dynamics_curve* curve, double level_db, double* gain_db, const char** why) {
    if (!curve || !gain_db) return dy_fail(why, "null pointer");
    if (!dy_table_ok(curve->T)) return dy_fail(why, "a table entry beyond OMX_DYNAMICS_MAX_GAIN");
    if (std::isnan(level_db)) return dy_fail(why, "a level that is NaN");
    const double l = std::floor(level_db / kDyOctave * 65536.0 + 0.5);
    const int32_t L = l <= (double)kDyLMin ? kDyLMin : (l >= (double)kDyLMax ? kDyLMax : (int32_t)l);
    *gain_db = (double)dy_curve_at(curve->T, L) * (kDyOctave / 65536.0);
    return OMX_NONE;
}

inline int dy_time(double fs, double attack_ms, double hold_ms, double release_db_per_s, uint32_t* attack, uint32_t* hold, int64_t* step,
                   const char** why) {
    if (!std::isfinite(fs) || !(fs > 0.0)) return dy_fail(why, "a sample rate that is not finite or not positive");
    if (!std::isfinite(attack_ms) || attack_ms < 0.0 || !std::isfinite(hold_ms) || hold_ms < 0.0)
        return dy_fail(why, "attack_ms or hold_ms negative or not finite");
    const double a = std::max(1.0, std::floor(attack_ms * fs / 1000.0 + 0.5)), h = std::floor(hold_ms * fs / 1000.0 + 0.5);
    if (a > (double)OMX_DYNAMICS_MAX_ATTACK) return dy_fail(why, "an attack beyond 4096 frames");
    if (h > (double)OMX_DYNAMICS_MAX_HOLD) return dy_fail(why, "a hold beyond 16384 frames");
    if (!(release_db_per_s > 0.0)) return dy_fail(why, "release_db_per_s not positive or NaN");
    const double d = std::floor(release_db_per_s / kDyOctave * 4294967296.0 / fs + 0.5);
    if (attack) *attack = (uint32_t)a;
    if (hold) *hold = (uint32_t)h;
    if (step) *step = d >= (double)OMX_DYNAMICS_MAX_STEP ? (int64_t)OMX_DYNAMICS_MAX_STEP : (d < 1.0 ? 1 : (int64_t)d);
    return OMX_NONE;
}

}  // namespace omx
