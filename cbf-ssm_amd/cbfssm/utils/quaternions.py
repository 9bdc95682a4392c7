"""cbfssm.utils.quaternions: the reference's quaternion helpers (cbfssm/utils/quaternions.py) with the same names and
conventions, on torch tensors (the reference's TensorFlow functions) or numpy arrays (its `_np` functions; here every
function takes either).  Quaternions are (..., 4) arrays, scalar part first; `multiply` is the Hamilton product
a (x) b; `invert` is the conjugate (the inverse of a UNIT quaternion); `rot_vec(v, q)` is the vector part of
q (x) (0, v) (x) conj(q), which rotates v when |q| = 1 and scales it by |q|^2 otherwise.

Plain tensor code for run scripts, outputs and data preparation: the filter loop of the Voliro model does not come
through here (cbfssm.hip.autograd.rigid_filter is a HIP kernel with the same conventions)."""
import numpy as np
import torch


def _is_torch(*xs):
    return any(torch.is_tensor(x) for x in xs)


def _stack(parts, like_torch):
    return torch.stack(parts, dim=-1) if like_torch else np.stack(parts, axis=-1)


class Quaternion:

    @staticmethod
    def multiply(a, b):
        """Hamilton product of (..., 4) quaternions, scalar first"""
        tt = _is_torch(a, b)
        if tt:
            a = a if torch.is_tensor(a) else torch.as_tensor(a, dtype=b.dtype, device=b.device)
            b = b if torch.is_tensor(b) else torch.as_tensor(b, dtype=a.dtype, device=a.device)
        else:
            a, b = np.asarray(a), np.asarray(b)
        a0, a1, a2, a3 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
        b0, b1, b2, b3 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
        return _stack((a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3,
                       a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                       a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1,
                       a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0), tt)

    @staticmethod
    def multiply_np(a, b):
        return Quaternion.multiply(np.asarray(a), np.asarray(b))

    @staticmethod
    def invert(a):
        """the conjugate"""
        if torch.is_tensor(a):
            return a * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=a.dtype, device=a.device)
        return np.asarray(a) * np.asarray([1.0, -1.0, -1.0, -1.0])

    @staticmethod
    def invert_np(a):
        return Quaternion.invert(np.asarray(a))

    @staticmethod
    def pad_to_quat(a):
        """(..., 3) vector -> (..., 4) quaternion with a zero scalar part"""
        if torch.is_tensor(a):
            return torch.cat((torch.zeros_like(a[..., 0:1]), a), dim=-1)
        a = np.asarray(a)
        return np.concatenate((np.zeros_like(a[..., 0:1]), a), axis=-1)

    @staticmethod
    def rot_vec(v, q):
        res = Quaternion.multiply(q, Quaternion.pad_to_quat(v))
        return Quaternion.multiply(res, Quaternion.invert(q))[..., 1:]
