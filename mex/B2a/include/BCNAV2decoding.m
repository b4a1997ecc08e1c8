function [eph, firstSubFrame, TOW] = BCNAV2decoding(I_P_InputBits)
% Drop-in for B2a/include/BCNAV2decoding.m on the GPU: preamble search, the five-chip
% vote per symbol, polarity by the preamble, CRC-24Q and the fields of message types
% 10, 11 and 30..34 of every message that passes, through bds_mex('nav_decode', ...)
% -> bds_nav_decode of libbds_mi355x.so.  No LDPC decoding, as in the reference.
%
%   [eph, firstSubFrame, TOW] = BCNAV2decoding(I_P_InputBits)
%
% eph has the fields of eph_structure_init ([] where nothing was decoded);
% firstSubFrame and TOW (= eph.SOW of the first message) are inf where no message
% passed.  A CRC-valid message whose PRN field is outside 1..63 is not entered.
out = bds_mex('nav_decode', 2, 1, double(I_P_InputBits(:).'), []);
eph = rmfield(out.eph, {'SOH', 'HOW', 'IODC', 'IODE', 'T_GDB2ap', 'ISC_B1Cd', 'T_GDB1Cp', ...
                        'PageID1', 'PageID3', 'SISMAI', 'TOW', 'flag', 'n_entered'});
types = {[], 'GEO', 'IGSO', 'MEO'};
eph.SatType = types{out.eph.SatType + 1};
firstSubFrame = out.firstSubFrame;
TOW = out.TOW;
end
