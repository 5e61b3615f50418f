"""The checker of observation / point filtering: a direct restatement of the reference's loops
(sfm/observation_manager.cc:311-326, 353-585, scene/projection.cc:40-141, geometry/triangulation.cc:217-249,
scene/reconstruction.cc:959-975) on a colmap_amd.scene.Reconstruction. It is SEQUENTIAL and deletes as it goes --
DeleteObservation takes the whole point when the track has length <= 2 at that moment -- and uses none of the closed
per-point forms of colmap_amd/csrc/obs_filter.hip, so the two are independent. Projection is scene.img_from_cam with the
validity rule of each model stated here; CamFromImg is the numpy restatement tests/undistort_reference.py already holds.

A `Trace` records what a test needs besides the filtered model: which rule deleted a point, the count a point
contributed, and the values decisions were taken on (observation errors, decisive triangulation angles, depths), so
that a generator can be checked to stay away from the thresholds."""
import numpy as np

import undistort_reference as R
from colmap_amd import scene

PIXEL, NORMALIZED, ANGULAR = 0, 1, 2
KEPT, DELETED_ERROR, DELETED_ANGLE, DELETED_SHORT, DELETED_DEPTH = range(5)
EPS = np.finfo(np.float64).eps
DBL_MAX = np.finfo(np.float64).max


class Trace:
    def __init__(self):
        self.status, self.count = {}, {}
        self.errors, self.angles, self.depths = [], [], []

    def add(self, pid, n):
        self.count[pid] = self.count.get(pid, 0) + n


def img_from_cam(cam, uvw):
    """Camera::ImgFromCam(uvw) with check_cheirality = true; None where the reference has no value (sensor/models.h)."""
    u, v, w = (float(x) for x in uvw)
    m, p = cam.model_id, np.asarray(cam.params, np.float64)
    if m == scene.EQUIRECTANGULAR:
        if np.sqrt(u * u + w * w) + abs(v) < EPS:
            return None
    elif m in (scene.SIMPLE_DIVISION, scene.DIVISION):
        if w * w - 4.0 * (u * u + v * v) * p[-1] < 0.0:
            return None
    else:
        if not w >= EPS:
            return None
        if m == scene.EUCM:
            rho2 = p[5] * (u * u + v * v) + w * w
            if rho2 < 0.0 or not p[4] * np.sqrt(rho2) + (1.0 - p[4]) * w >= EPS:
                return None
    return scene.img_from_cam(m, p, np.array([[u, v, w]]))[0]


def cam_ray_from_img(cam, xy):
    """Camera::CamRayFromImg: unit bearing, None where CamFromImg has no value."""
    p = np.asarray(cam.params, np.float64)
    if cam.model_id == scene.EQUIRECTANGULAR:
        theta = 2.0 * np.pi * (xy[0] / p[0] - 0.5)
        phi = np.pi * (0.5 - xy[1] / p[1])
        return np.array([np.cos(phi) * np.sin(theta), -np.sin(phi), np.cos(phi) * np.cos(theta)])
    uv = R.cam_from_img(R.Camera(cam.model_id, cam.width, cam.height, p), np.asarray(xy, np.float64)[None])[0]
    if np.isnan(uv).any():
        return None
    ray = np.array([uv[0], uv[1], 1.0])
    return ray / np.sqrt(uv[0] * uv[0] + uv[1] * uv[1] + 1.0)


def _normalized(v):
    n2 = float(v @ v)
    return v / np.sqrt(n2) if n2 > 0.0 else v


def point_in_cam(img, xyz):
    return scene.quat_to_rot(img.cam_from_world[:4]) @ xyz + img.cam_from_world[4:]


def angular_reprojection_error(xy, xyz, img, cam):
    ray = cam_ray_from_img(cam, xy)
    if ray is None:
        return np.pi
    return float(np.arccos(np.clip(ray @ _normalized(point_in_cam(img, xyz)), -1.0, 1.0)))


def squared_reprojection_error(xy, xyz, img, cam):
    if cam.model_id == scene.EQUIRECTANGULAR:
        pixel_error = angular_reprojection_error(xy, xyz, img, cam) * (cam.width / (2.0 * np.pi))
        return pixel_error * pixel_error
    proj = img_from_cam(cam, point_in_cam(img, xyz))
    if proj is None:
        return DBL_MAX
    d = proj - xy
    return float(d @ d)


def observation_error(rec, pid, image_id, idx, error_type):
    img = rec.images[image_id]
    cam = rec.cameras[img.camera_id]
    xy, xyz = img.points2D[idx].xy, rec.points3D[pid].xyz
    if error_type == PIXEL:
        return float(np.sqrt(squared_reprojection_error(xy, xyz, img, cam)))
    if error_type == NORMALIZED:
        pc = point_in_cam(img, xyz)
        if cam.model_id != scene.EQUIRECTANGULAR:
            uv = R.cam_from_img(R.Camera(cam.model_id, cam.width, cam.height, cam.params), np.asarray(xy, np.float64)[None])[0]
            if pc[2] >= 1e-12 and not np.isnan(uv).any():
                return float(np.linalg.norm(pc[:2] / pc[2] - uv))
            return float("inf")
        ray = cam_ray_from_img(cam, xy)
        return float(np.linalg.norm(_normalized(pc) - ray)) if ray is not None else float("inf")
    return float(np.rad2deg(angular_reprojection_error(xy, xyz, img, cam)))


def triangulation_angle(c1, c2, xyz):
    v1, v2 = xyz - c1, xyz - c2
    n1, n2 = float(v1 @ v1), float(v2 @ v2)
    angle = 0.0 if n1 == 0.0 or n2 == 0.0 else float(np.arccos(np.clip((v1 @ v2) / np.sqrt(n1 * n2), -1.0, 1.0)))
    return min(angle, np.pi - angle)


def _delete_point(rec, pid, trace, status):
    if trace is not None:
        trace.status[pid] = status
    rec.DeletePoint3D(pid)


def DeleteObservation(rec, image_id, idx, trace=None, status=KEPT):
    """ObservationManager::DeleteObservation (:311-326)."""
    pid = rec.images[image_id].points2D[idx].point3D_id
    pt = rec.points3D[pid]
    if len(pt.track) <= 2:
        _delete_point(rec, pid, trace, status)
        return
    pt.track.remove((image_id, idx))
    rec.images[image_id].points2D[idx].point3D_id = -1


def FilterPoints3DWithLargeReprojectionError(rec, max_error, point3D_ids, error_type=PIXEL, trace=None):
    n = 0
    for pid in point3D_ids:
        if pid not in rec.points3D:
            continue
        pt = rec.points3D[pid]
        if len(pt.track) < 2:
            n += len(pt.track)
            if trace is not None:
                trace.add(pid, len(pt.track))
            _delete_point(rec, pid, trace, DELETED_ERROR)
            continue
        error_sum, to_delete = 0.0, []
        for (im, idx) in pt.track:
            e = observation_error(rec, pid, im, idx, error_type)
            if trace is not None:
                trace.errors.append(e)
            if e > max_error:
                to_delete.append((im, idx))
            else:
                error_sum += e
        if len(to_delete) >= len(pt.track) - 1:
            n += len(pt.track)
            if trace is not None:
                trace.add(pid, len(pt.track))
            _delete_point(rec, pid, trace, DELETED_ERROR)
        else:
            n += len(to_delete)
            if trace is not None:
                trace.add(pid, len(to_delete))
            for (im, idx) in to_delete:
                DeleteObservation(rec, im, idx, trace, DELETED_ERROR)
            pt.error = error_sum / len(pt.track)
    return n


def FilterPoints3DWithSmallTriangulationAngle(rec, min_tri_angle, point3D_ids, trace=None):
    n = 0
    min_rad = np.deg2rad(min_tri_angle)
    centers = {}
    for pid in point3D_ids:
        if pid not in rec.points3D:
            continue
        pt = rec.points3D[pid]
        keep, largest = False, -1.0
        for i1 in range(len(pt.track)):
            im1 = pt.track[i1][0]
            if im1 not in centers:
                centers[im1] = rec.ProjectionCenter(im1)
            for i2 in range(i1):
                a = triangulation_angle(centers[im1], centers[pt.track[i2][0]], pt.xyz)
                largest = max(largest, a)
                if a >= min_rad and trace is None:
                    keep = True
                    break
                keep = keep or a >= min_rad  # with a trace every pair is visited: the decisive angle is the largest
            if keep and trace is None:
                break
        if trace is not None and largest >= 0.0:
            trace.angles.append(largest)
        if not keep:
            n += len(pt.track)
            if trace is not None:
                trace.add(pid, len(pt.track))
            _delete_point(rec, pid, trace, DELETED_ANGLE)
    return n


def FilterPoints3D(rec, max_reproj_error, min_tri_angle, point3D_ids, error_type=PIXEL, trace=None):
    ids = list(point3D_ids)
    return FilterPoints3DWithLargeReprojectionError(rec, max_reproj_error, ids, error_type, trace) + \
        FilterPoints3DWithSmallTriangulationAngle(rec, min_tri_angle, ids, trace)


def FilterPoints3DInImages(rec, max_reproj_error, min_tri_angle, image_ids, trace=None):
    ids = []
    for image_id in image_ids:
        ids += [p.point3D_id for p in rec.images[image_id].points2D if p.HasPoint3D()]
    return FilterPoints3D(rec, max_reproj_error, min_tri_angle, list(dict.fromkeys(ids)), trace=trace)


def FilterAllPoints3D(rec, max_reproj_error, min_tri_angle, error_type=PIXEL, trace=None):
    return FilterPoints3D(rec, max_reproj_error, min_tri_angle, list(rec.points3D), error_type, trace)


def FilterPoints3DWithShortTracks(rec, min_track_length, trace=None):
    n = 0
    for pid in list(rec.points3D):
        pt = rec.points3D[pid]
        if len(pt.track) < min_track_length:
            n += len(pt.track)
            if trace is not None:
                trace.add(pid, len(pt.track))
            _delete_point(rec, pid, trace, DELETED_SHORT)
    return n


def FilterObservationsWithNegativeDepth(rec, trace=None):
    n = 0
    for image_id in rec.RegImageIds():
        img = rec.images[image_id]
        if rec.cameras[img.camera_id].model_id == scene.EQUIRECTANGULAR:
            continue
        row2 = scene.quat_to_rot(img.cam_from_world[:4])[2]
        for idx, p2 in enumerate(img.points2D):
            if p2.HasPoint3D():
                pid = p2.point3D_id
                depth = float(row2 @ rec.points3D[pid].xyz + img.cam_from_world[6])
                if trace is not None:
                    trace.depths.append(depth)
                if not depth >= EPS:
                    if trace is not None:
                        trace.add(pid, 1)
                    DeleteObservation(rec, image_id, idx, trace, DELETED_DEPTH)
                    n += 1
    return n


def UpdatePoint3DErrors(rec):
    for pid, pt in rec.points3D.items():
        if not pt.track:
            pt.error = 0.0
            continue
        e = 0.0
        for (im, idx) in pt.track:
            img = rec.images[im]
            e += np.sqrt(squared_reprojection_error(img.points2D[idx].xy, pt.xyz, img, rec.cameras[img.camera_id]))
        pt.error = float(e / len(pt.track))


class Manager:
    """The checker behind the method names of ObservationManager (stands in for the library in the command's tests)."""

    def __init__(self, rec, gpu_index=0):
        self.rec = rec

    def FilterPoints3D(self, e, a, ids):
        return FilterPoints3D(self.rec, e, a, ids)

    def FilterPoints3DInImages(self, e, a, image_ids):
        return FilterPoints3DInImages(self.rec, e, a, image_ids)

    def FilterAllPoints3D(self, e, a):
        return FilterAllPoints3D(self.rec, e, a)

    def FilterPoints3DWithShortTracks(self, n):
        return FilterPoints3DWithShortTracks(self.rec, n)

    def FilterPoints3DWithLargeReprojectionError(self, e, ids, error_type=PIXEL):
        return FilterPoints3DWithLargeReprojectionError(self.rec, e, list(ids), error_type)

    def FilterPoints3DWithSmallTriangulationAngle(self, a, ids):
        return FilterPoints3DWithSmallTriangulationAngle(self.rec, a, list(ids))

    def FilterObservationsWithNegativeDepth(self):
        return FilterObservationsWithNegativeDepth(self.rec)
