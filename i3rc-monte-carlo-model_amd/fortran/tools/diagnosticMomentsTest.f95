! Batch moments of the diagnostic tallies through the Fortran shell: computeRadiativeTransferDiagnosticMoments and
! reportDiagnosticMoments on the small cloud of levelFluxTest, six batches of 5000 photons with the seeds (/ 7, 3 ... 8 /), first with
! the level fluxes, then with the actinic flux.  Prints the sums and sums of squares over the batches -- per level (layer) those of the
! domain means and of every column -- for tests/test_gpu_diagnostic_moments.py, which runs the same loop through the Python mirror, and
! what the shell answers when moments are asked for that were not computed, into arrays of the wrong shape, or after the kind changed.
program diagnosticMomentsTest
  use ErrorMessages
  use scatteringPhaseFunctions
  use opticalProperties
  use monteCarloRadiativeTransfer
  implicit none
  integer, parameter :: nx = 4, ny = 2, nz = 6, nPhotons = 5000, nBatches = 6, iseed = 7, firstBatch = 3
  type(ErrorMessage)       :: status
  type(domain)             :: cloud
  type(integrator)         :: mc
  type(phaseFunction)      :: hg
  type(phaseFunctionTable) :: table
  real    :: ext(nx, ny, nz), ssa(nx, ny, nz)
  real    :: up(nx, ny, nz + 1, 2), down(nx, ny, nz + 1, 2), meanUp(nz + 1, 2), meanDown(nz + 1, 2)
  real    :: actinic(nx, ny, nz, 2), meanActinic(nz, 2), wrong(nx, ny, nz, 2), wrongMean(nz, 2), meanFluxUp(2), meanFluxDown(2)
  integer :: idx(nx, ny, nz), i, j, k, m, batches

  hg = new_PhaseFunction(0.85**(/ (i, i = 1, 64) /), status = status)
  table = new_PhaseFunctionTable((/ hg /), key = (/ 1. /), status = status)
  do k = 1, nz
    do j = 1, ny
      do i = 1, nx
        ext(i, j, k) = 0.0002
        if(k >= 3 .and. k <= 5) ext(i, j, k) = 0.004 * (1 + mod(i + j, 3))
      end do
    end do
  end do
  ssa = 0.95; idx = 1
  cloud = new_Domain((/ 0., 500., 1000., 1500., 2000. /), (/ 0., 500., 1000. /), (/ 0., 100., 250., 300., 500., 800., 1000. /), status)
  call addOpticalComponent(cloud, "cloud", ext, ssa, idx, table, status = status)
  mc = new_Integrator(cloud, status)
  if(stateIsFailure(status)) then
    print *, "new_Integrator failed"; stop 1
  end if
  call specifyParameters(mc, surfaceAlbedo = 0.3, minInverseTableSize = 10001, status = status)

  ! nothing computed yet; no diagnostic switched on
  call initializeState(status)
  call reportDiagnosticMoments(mc, meanLevelFluxUpStats = meanUp, status = status)
  print '(a, l2, 1x, a)', "nothingyet  ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call computeRadiativeTransferDiagnosticMoments(mc, iseed, firstBatch, nBatches, 0.5, 30., nPhotons, status)
  print '(a, l2, 1x, a)', "switchedoff ", stateIsFailure(status), trim(failureText())
  call initializeState(status)

  ! -- level fluxes
  call specifyParameters(mc, status = status, computeLevelFluxes = .true.)
  call computeRadiativeTransferDiagnosticMoments(mc, iseed, firstBatch, nBatches, 0.5, 30., nPhotons, status)
  if(stateIsFailure(status)) then
    print *, "computeRadiativeTransferDiagnosticMoments failed: ", trim(failureText()); stop 1
  end if
  call initializeState(status)
  call reportDiagnosticMoments(mc, levelFluxUpStats = wrong, status = status)
  print '(a, l2, 1x, a)', "wrongshape  ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call reportDiagnosticMoments(mc, meanLevelFluxDownStats = wrongMean, status = status)
  print '(a, l2, 1x, a)', "wrongmean   ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call reportDiagnosticMoments(mc, actinicFluxStats = actinic, status = status)
  print '(a, l2, 1x, a)', "unavailable ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call reportDiagnosticMoments(mc, levelFluxUpStats = up, levelFluxDownStats = down, meanLevelFluxUpStats = meanUp, &
                               meanLevelFluxDownStats = meanDown, status = status)
  if(stateIsFailure(status)) then
    print *, "reportDiagnosticMoments failed: ", trim(failureText()); stop 1
  end if
  call reportBatchMoments(mc, numBatches = batches, meanFluxUpStats = meanFluxUp, meanFluxDownStats = meanFluxDown, status = status)
  print '(a, i4)', "batches     ", batches
  print '(a, 4es16.8)', "meanflux    ", meanFluxUp, meanFluxDown
  do m = 1, 2
    do k = 1, nz + 1
      print '(a, 2i3, es16.8)',  "meanup   ", m, k - 1, meanUp(k, m)
      print '(a, 2i3, es16.8)',  "meandown ", m, k - 1, meanDown(k, m)
      print '(a, 2i3, 8es16.8)', "levelup  ", m, k - 1, ((up(i, j, k, m), i = 1, nx), j = 1, ny)
      print '(a, 2i3, 8es16.8)', "leveldown", m, k - 1, ((down(i, j, k, m), i = 1, nx), j = 1, ny)
    end do
  end do

  ! the kind changes between the computation and the report
  call specifyParameters(mc, status = status, computeLevelFluxes = .false.)
  call initializeState(status)
  call reportDiagnosticMoments(mc, meanLevelFluxUpStats = meanUp, status = status)
  print '(a, l2, 1x, a)', "switchedoff2", stateIsFailure(status), trim(failureText())
  call specifyParameters(mc, status = status, computeActinicFlux = .true.)
  call initializeState(status)
  call reportDiagnosticMoments(mc, meanLevelFluxUpStats = meanUp, status = status)
  print '(a, l2, 1x, a)', "otherkind   ", stateIsFailure(status), trim(failureText())
  call initializeState(status)

  ! -- the actinic flux
  call computeRadiativeTransferDiagnosticMoments(mc, iseed, firstBatch, nBatches, 0.5, 30., nPhotons, status)
  if(stateIsFailure(status)) then
    print *, "computeRadiativeTransferDiagnosticMoments failed: ", trim(failureText()); stop 1
  end if
  call initializeState(status)
  call reportDiagnosticMoments(mc, levelFluxDownStats = down, status = status)
  print '(a, l2, 1x, a)', "unavailable2", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call reportDiagnosticMoments(mc, actinicFluxStats = actinic, meanActinicFluxStats = meanActinic, status = status)
  if(stateIsFailure(status)) then
    print *, "reportDiagnosticMoments failed: ", trim(failureText()); stop 1
  end if
  do m = 1, 2
    do k = 1, nz
      print '(a, 2i3, es16.8)',  "meanactinic", m, k - 1, meanActinic(k, m)
      print '(a, 2i3, 8es16.8)', "actinic    ", m, k - 1, ((actinic(i, j, k, m), i = 1, nx), j = 1, ny)
    end do
  end do
  ! an ordinary loop afterwards forgets the diagnostic moments
  call specifyParameters(mc, status = status, computeActinicFlux = .false.)
  call computeRadiativeTransferBatchMoments(mc, iseed, firstBatch, 2, 0.5, 30., nPhotons, status)
  call initializeState(status)
  call reportDiagnosticMoments(mc, meanActinicFluxStats = meanActinic, status = status)
  print '(a, l2, 1x, a)', "forgotten   ", stateIsFailure(status), trim(failureText())
  call finalize_Integrator(mc)
  print '(a)', "diagnostic moments test done"
contains
  ! the newest message of the status object that says something (the probes start from a fresh one; a computation leaves the
  ! successes of its preparations in front of its failure)
  function failureText() result(text)
    character(len = 256) :: text, line
    text = ""
    call firstMessage(status)
    do while(moreMessagesExist(status))
      line = getCurrentMessage(status)
      if(len_trim(line) > 0) text = line
      call nextMessage(status)
    end do
  end function failureText
end program diagnosticMomentsTest
