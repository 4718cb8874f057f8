"""Restatement of the failure-prediction classifier and of the policy it drives, independent of the
library: cv::ml::SVM::predict(..., RAW_OUTPUT) of a two-class C_SVC with a POLY kernel and the
logistic of aicp_core/src/classification/svm.cpp:82, the reader of the model XML, the writer of the
test models, App's stream policy with the risk gate (app.cpp:362-414) as a state machine, and App's
corrected pose (aligned_cloud.cpp:31-74, common.cpp:4-23, 70-105) in double.

The arithmetic, per sample x and support vector v:
  s = (double)(v0 * x0) + (double)(v1 * x1), the products in float32;
  base = (float32)(s * gamma + coef0);  K = (float32)pow((double)base, degree);
  sum = -rho + sum_j alpha[j] * K[index[j]] in double, j ascending;  raw = (float32)sum;
  risk = 1 - 1 / (1 + exp(-(double)raw)).
"""
import math
import os
import xml.etree.ElementTree as ET

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svm")
MODELS = {
    # name -> (model file, recording, samples above 0.5 in the recording)
    "opencv3": ("svm_1000training_thresh50_cross_validation_opencv3.xml", "probs_opencv3.txt", 81),
    "thresh60": ("svm_1000training_thresh60.xml", "probs_27Aug.txt", 141),
}
INPUTS = "testing_labelled_27Aug.txt"


def golden(name):
    return os.path.join(GOLDEN, name)


def read_model(path):
    """The model XML through ElementTree: both root forms, an absent <index> is the identity."""
    root = ET.parse(path).getroot()
    node = root.find("opencv_ml_svm")
    fmt = 3
    if node is None:
        node, fmt = root.find("my_svm"), 0
    assert node is not None, "no svm root"
    typ = node.find("svmType") if node.find("svmType") is not None else node.find("svm_type")
    k = node.find("kernel")
    sv = np.array([[np.float32(t) for t in row.text.split()] for row in node.find("support_vectors").findall("_")],
                  np.float32)
    df = node.find("decision_functions").find("_")
    alpha = np.array([float(t) for t in df.find("alpha").text.split()], np.float64)
    idx = df.find("index")
    index = np.arange(len(alpha), dtype=np.int32) if idx is None else np.array(idx.text.split(), np.int32)
    return dict(format=fmt, svm_type=typ.text.strip(), kernel=k.find("type").text.strip(),
                degree=float(k.find("degree").text), gamma=float(k.find("gamma").text),
                coef0=float(k.find("coef0").text), var_count=int(node.find("var_count").text),
                class_count=int(node.find("class_count").text), sv_total=int(node.find("sv_total").text),
                sv_count=int(df.find("sv_count").text), rho=float(df.find("rho").text), has_index=int(idx is not None),
                support_vectors=sv, alpha=alpha, index=index)


def read_inputs(path=None):
    """testing_labelled_27Aug.txt: rows `id overlap alignability label` -> (n, 2) float32 samples as
    the classifier takes them. The file holds the alignability as a fraction; App's alignability_ is
    in percent (app.cpp:169; the models' support vectors reach 90 in that coordinate), and the
    recordings were computed from percent: a cubic fitted to the recorded values of the degree-3
    model has the model's own coefficients only with the second column times 100."""
    rows = [ln.split() for ln in open(path or golden(INPUTS)) if ln.strip()]
    return np.array([[float(r[1]), 100.0 * float(r[2])] for r in rows]).astype(np.float32)


def read_probs(path):
    """A recording: rows `id probability`; the values and their text (for the print rounding)."""
    rows = [ln.split() for ln in open(path) if ln.strip()]
    return np.array([float(r[1]) for r in rows]), [r[1] for r in rows]


def print_half_unit(text):
    """Half a unit of the sixth significant digit of a printed value (the stream's default
    precision; trailing zeros are not printed, so the text's length does not tell)."""
    v = abs(float(text))
    return 0.5 * 10.0 ** (math.floor(math.log10(v)) - 5)


def ulp32(x):
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def predict(m, X):
    """raw float32[n], risk float64[n], and terms[n, sv_count] = alpha_j * K_j (double) for the bars."""
    X = np.asarray(X, np.float32).reshape(-1, 2)
    v = m["support_vectors"][m["index"]]                       # decision-function order
    p0 = (v[None, :, 0] * X[:, None, 0]).astype(np.float32)    # float products
    p1 = (v[None, :, 1] * X[:, None, 1]).astype(np.float32)
    s = p0.astype(np.float64) + p1.astype(np.float64)
    base = (s * m["gamma"] + m["coef0"]).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        K = np.power(base.astype(np.float64), m["degree"]).astype(np.float32)
    terms = m["alpha"][None, :] * K.astype(np.float64)
    total = np.full(len(X), -m["rho"], np.float64)
    for j in range(terms.shape[1]):                            # j ascending, in double
        total = total + terms[:, j]
    raw = total.astype(np.float32)
    with np.errstate(over="ignore"):
        risk = 1.0 - 1.0 / (1.0 + np.exp(-raw.astype(np.float64)))
    return raw, risk, terms


def raw_bar(raw_ref, terms):
    """|raw_dev - raw_ref| <= ulp32(raw_ref) + 2^-23 max_k |alpha_k| K_k: the one float rounding of the
    sum, and one K on the neighbouring float."""
    return ulp32(raw_ref) + 2.0 ** -23 * np.abs(terms).max(axis=1)


def recorded_bar(raw_ref, terms, texts):
    """|risk_dev - recorded| <= half a unit of the recorded value's last printed digit + 1/4 (ulp32(raw)
    + 2^-23 sum_k |alpha_k| K_k): the print rounding, and the float roundings of raw and of every K
    through the logistic, whose slope is at most 1/4."""
    half = np.array([print_half_unit(t) for t in texts])
    return half + 0.25 * (ulp32(raw_ref) + 2.0 ** -23 * np.abs(terms).sum(axis=1))


def gate(risk, threshold):
    """!(risk <= threshold): a NaN risk gates, as in C++ (app.cpp:244, 363)."""
    return ~(np.asarray(risk, np.float64) <= threshold)


# ---- model files the tests write ----------------------------------------------------------------
def write_model(path, sv, alpha, rho, degree, gamma, coef0, index="identity", fmt=3, svm_type="C_SVC", kernel="POLY",
                class_count=2, var_count=None, sv_total=None, sv_count=None, truncate=None):
    """An OpenCV SVM model file in either root form. index: "identity" writes 0..n-1, None writes no
    <index>, else the given entries. truncate: keep only that many characters."""
    sv = np.asarray(sv, np.float32)
    alpha = np.asarray(alpha, np.float64)
    var_count = sv.shape[1] if var_count is None else var_count
    sv_total = len(sv) if sv_total is None else sv_total
    sv_count = len(alpha) if sv_count is None else sv_count
    rows = "".join("    <_>\n      %s</_>\n" % " ".join("%.8e" % float(x) for x in r) for r in sv)
    al = " ".join(repr(float(a)) for a in alpha)
    if isinstance(index, str):
        index = list(range(len(alpha)))
    ix = "" if index is None else "      <index>\n        %s</index>" % " ".join(str(int(i)) for i in index)
    kern = ("  <kernel>\n    <type>%s</type>\n" % kernel +
            ("    <degree>%r</degree>\n" % float(degree) if kernel == "POLY" else "") +
            "    <gamma>%r</gamma>\n" % float(gamma) +
            ("    <coef0>%r</coef0>" % float(coef0) if kernel == "POLY" else "") + "</kernel>\n")
    head = ("<opencv_ml_svm>\n  <format>3</format>\n  <svmType>%s</svmType>\n" % svm_type if fmt == 3 else
            '<my_svm type_id="opencv-ml-svm">\n  <svm_type>%s</svm_type>\n' % svm_type)
    tail = "</opencv_ml_svm>\n" if fmt == 3 else "</my_svm>\n"
    labels = " ".join(str(i) for i in range(class_count))
    doc = ('<?xml version="1.0"?>\n<opencv_storage>\n' + head + kern +
           "  <C>1.</C>\n  <term_criteria><iterations>100</iterations></term_criteria>\n"
           "  <var_count>%d</var_count>\n  <class_count>%d</class_count>\n" % (var_count, class_count) +
           '  <class_labels type_id="opencv-matrix">\n    <rows>%d</rows>\n    <cols>1</cols>\n    <dt>i</dt>\n'
           "    <data>\n      %s</data></class_labels>\n" % (class_count, labels) +
           "  <sv_total>%d</sv_total>\n  <support_vectors>\n%s</support_vectors>\n" % (sv_total, rows.rstrip("\n")) +
           "  <decision_functions>\n    <_>\n      <sv_count>%d</sv_count>\n      <rho>%r</rho>\n"
           "      <alpha>\n        %s</alpha>\n%s</_></decision_functions>" % (sv_count, float(rho), al, ix) + tail +
           "</opencv_storage>\n")
    if truncate is not None:
        doc = doc[:truncate]
    with open(path, "w") as f:
        f.write(doc)
    return path


def write_threshold_model(path, X):
    """degree 1, gamma 1, coef0 0, one support vector (1, 0), alpha 1, rho X: raw = overlap - X, so
    risk > 0.5 <=> raw < 0 <=> overlap < X."""
    return write_model(path, [[1.0, 0.0]], [1.0], X, 1.0, 1.0, 0.0)


# ---- App's stream policy with the gate (app.cpp:362-414) ------------------------------------------
class GatePolicy:
    """What App keeps between readings, without any cloud: the current reference, the count of
    accepted readings since the last reference, initialT_ (debug mode). step() takes one reading's
    risk and correction and returns its flags."""

    def __init__(self, frequency, max_correction, threshold):
        self.F, self.max_corr, self.thr = int(frequency), np.float32(max_correction), float(threshold)
        self.reference, self.acc = -1, 0
        self.initT = np.eye(4, dtype=np.float32)
        self.graph = [-1]  # clouds in the aligned-cloud graph: the first cloud, then reading indices

    def gated(self, risk):
        return not (risk <= self.thr)

    def step(self, i, risk, T):
        """T: the correction (4x4 float32; ignored for a gated reading). Returns dict(reference,
        registered, accepted, is_reference)."""
        out = dict(reference=self.reference, registered=0, accepted=0, is_reference=0)
        if self.gated(risk):  # app.cpp:401-411
            self.graph.append(i)
            self.reference, self.acc = i, 0
            out.update(accepted=1, is_reference=1)
            return out  # correction = identity: initialT_ unchanged
        out["registered"] = 1
        T = np.asarray(T, np.float32)
        if (np.abs(T[:3, 3]) > self.max_corr).any():  # app.cpp:366-373: a drop changes nothing
            return out
        out["accepted"] = 1
        self.graph.append(i)
        self.acc += 1
        if self.acc == self.F:  # app.cpp:383-391
            self.reference, self.acc = i, 0
            out["is_reference"] = 1
        self.initT = mul4f(T, self.initT)  # app.cpp:414
        return out


def mul4f(A, B):
    """4x4 float32 product, each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3 in float32 (the library's mul4)."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    out = np.zeros((4, 4), np.float32)
    for r in range(4):
        for c in range(4):
            acc = np.float32(A[r, 0] * B[0, c])
            for k in range(1, 4):
                acc = np.float32(acc + np.float32(A[r, k] * B[k, c]))
            out[r, c] = acc
    return out


# ---- App's corrected pose in double (math = libm, as the library's host code) ---------------------
def _quat_from_rotation(m, sqrt=math.sqrt, one=1.0, half=0.5):
    t = (m[0][0] + m[1][1]) + m[2][2]
    q = [0, 0, 0, 0]  # x, y, z, w
    if t > 0:
        t = sqrt(t + one)
        q[3] = half * t
        t = half / t
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = sqrt(((m[i][i] - m[j][j]) - m[k][k]) + one)
        q[i] = half * t
        t = half / t
        q[3] = (m[k][j] - m[j][k]) * t
        q[j] = (m[j][i] + m[i][j]) * t
        q[k] = (m[k][i] + m[i][k]) * t
    return q


def _rotation_from_quat(q):
    x, y, z, w = (float(v) for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def _euler_from_quat(q):
    q1, q2, q3, q0 = q
    roll = math.atan2(2 * (q0 * q1 + q2 * q3), 1 - 2 * (q1 * q1 + q2 * q2))
    pitch = math.asin(2 * (q0 * q2 - q3 * q1))
    yaw = math.atan2(2 * (q0 * q3 + q1 * q2), 1 - 2 * (q2 * q2 + q3 * q3))
    return roll, pitch, yaw


def _quat_from_euler(roll, pitch, yaw):
    if roll == math.pi and pitch == 0 and yaw == 0:
        return [1.0, 0.0, 0.0, 0.0]
    if pitch == math.pi and roll == 0 and yaw == 0:
        return [0.0, 1.0, 0.0, 0.0]
    if yaw == math.pi and roll == 0 and pitch == 0:
        return [0.0, 0.0, 1.0, 0.0]
    sy, cy = math.sin(yaw * 0.5), math.cos(yaw * 0.5)
    sp, cp = math.sin(pitch * 0.5), math.cos(pitch * 0.5)
    sr, cr = math.sin(roll * 0.5), math.cos(roll * 0.5)
    return [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
            cr * cp * cy + sr * sp * sy]


def moved_pose(T, prior):
    """fromMatrix4fToIsometry3d(T) * prior: the float quaternion of T's rotation (its square root the
    correctly rounded float one), cast to double, times the 4x4 row-major double pose."""
    T = np.asarray(T, np.float32)
    f = np.float32
    q = _quat_from_rotation([[f(T[r, c]) for c in range(3)] for r in range(3)],
                            sqrt=lambda v: f(math.sqrt(float(v))), one=f(1), half=f(0.5))
    R = _rotation_from_quat(q)
    P = [[float(prior[r][c]) for c in range(4)] for r in range(4)]
    out = np.eye(4)
    for r in range(3):
        for c in range(3):
            out[r, c] = (R[r][0] * P[0][c] + R[r][1] * P[1][c]) + R[r][2] * P[2][c]
        out[r, 3] = ((R[r][0] * P[0][3] + R[r][1] * P[1][3]) + R[r][2] * P[2][3]) + float(T[r, 3])
    return out


def fix_pitch_roll(corrected, odom):
    """AlignedCloud::removePitchRollCorrection: translation and yaw of `corrected`, roll and pitch of
    the odometry pose."""
    tolist = lambda P: [[float(P[r][c]) for c in range(3)] for r in range(3)]
    ro, po, _ = _euler_from_quat(_quat_from_rotation(tolist(odom)))
    _, _, yc = _euler_from_quat(_quat_from_rotation(tolist(corrected)))
    out = np.eye(4)
    out[:3, :3] = np.array(_rotation_from_quat(_quat_from_euler(ro, po, yc)))
    out[:3, 3] = [float(corrected[r][3]) for r in range(3)]
    return out
