function report = notchTones(fileIn, fileOut, settings, freqs, blockLog2)
% Excision of narrow-band (CW) interference from an IF record file on the GPU, to be
% run on the record BEFORE acquisition and tracking read it:
%
%   report = notchTones(fileIn, fileOut, settings, freqs)
%   report = notchTones(fileIn, fileOut, settings, freqs, blockLog2)
%
% freqs holds up to 8 frequencies in Hz on probeData's axis: 0 .. fs/2 for a real
% record (settings.fileType 1), the IF included; signed baseband frequencies for an
% I/Q record.  Per block of 2^blockLog2 samples (default 10; 8 .. 16) the complex
% amplitude of every tone is estimated and the tone subtracted in fileOut; every
% other byte is fileIn's, the bytes in front of settings.skipNumberOfBytes included,
% so the same settings read both files (settings.fileName = fileOut afterwards).
% One notch is samplingFreq / 2^blockLog2 wide; two tones must lie four widths
% apart, and a tone of a real record two widths inside (0, fs/2).
% settings.skipNumberOfBytes counts samples, as in tracking.  Not for fileType 3.
%
% report: n_samples, n_blocks, n_saturated, sum_sq_in, sum_sq_out (the power
% before and after), steps (the phase steps applied) and est_re, est_im
% (n_blocks x n_tones: every tone's amplitude per block in LSB).
if ~ischar(fileIn) || ~ischar(fileOut), error('File name must be a string'); end
if nargin < 5 || isempty(blockLog2), blockLog2 = 10; end
signal = 2 - isfield(settings, 'acqCohT');   % only B1C/initSettings.m defines acqCohT: 1 = B1C, 2 = B2a
report = bds_mex('notch_tones', fileIn, fileOut, settings, signal, double(freqs(:).'), blockLog2);
fprintf('notchTones: %d tones, %d blocks, %.1f dB removed, %d samples saturated\n', ...
        numel(report.steps), report.n_blocks, 10 * log10(report.sum_sq_in / max(report.sum_sq_out, 1)), report.n_saturated);
end
